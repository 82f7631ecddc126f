"""TEST INFRASTRUCTURE: a numpy restatement of what csrc/png.hip computes, written from the rules in include/spaa_hip.h (not from
the kernel): the per-row PNG filter choice with the byte histogram and the Adler-32 row sums, and the deflate bit packer."""
import numpy as np


def to_bytes(x):
    """float32 [N,3,H,W] in [0,1] -> uint8, `np.uint8(x * 255)`: one fp32 multiply, truncation."""
    return np.uint8(np.asarray(x, dtype=np.float32) * np.float32(255))


def filter_image(img):
    """img uint8 [H,W,3] -> (stream uint8 [H, 1 + 3 W], hist int64 [257], rows int64 [H,2]).  All five filters from the unfiltered
    neighbours (0 outside the image), cost min(v, 256 - v) per byte, lowest row sum wins, ties to the lowest filter number.
    hist[256] = 1; rows = (sum of the row's bytes, sum of byte j times (row length - j)), exact."""
    h, w, _ = img.shape
    cur_all = img.reshape(h, 3 * w).astype(np.int64)
    stream = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
    rows = np.zeros((h, 2), dtype=np.int64)
    length = 1 + 3 * w
    weight = length - np.arange(length, dtype=np.int64)
    for y in range(h):
        x = cur_all[y]
        b = cur_all[y - 1] if y else np.zeros_like(x)
        a = np.concatenate([np.zeros(3, np.int64), x[:-3]])
        c = np.concatenate([np.zeros(3, np.int64), b[:-3]])
        pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        cands = [(x - p) & 255 for p in (0, a, b, (a + b) >> 1, paeth)]
        costs = [int(np.minimum(v, 256 - v).sum()) for v in cands]
        k = costs.index(min(costs))
        stream[y, 0] = k
        stream[y, 1:] = cands[k]
        line = stream[y].astype(np.int64)
        rows[y] = line.sum(), (line * weight).sum()
    hist = np.bincount(stream.reshape(-1), minlength=257).astype(np.int64)
    hist[256] = 1
    return stream, hist, rows


def filter_costs(img, y):
    """The five row costs of row y (for tests that need a tie)."""
    h, w, _ = img.shape
    rows = img.reshape(h, 3 * w).astype(np.int64)
    x = rows[y]
    b = rows[y - 1] if y else np.zeros_like(x)
    a = np.concatenate([np.zeros(3, np.int64), x[:-3]])
    c = np.concatenate([np.zeros(3, np.int64), b[:-3]])
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return [int(np.minimum((x - p) & 255, 256 - ((x - p) & 255)).sum()) for p in (0, a, b, (a + b) >> 1, paeth)]


def symbol_bit_starts(stream, lengths, header_bits):
    """Bit position (from the start of the image's deflate stream) of every symbol's code, the end of block last."""
    sym = np.concatenate([np.asarray(stream).reshape(-1).astype(np.int64), [256]])
    ln = np.asarray(lengths, dtype=np.int64)[sym]
    return header_bits + np.cumsum(ln) - ln


def pack_image(stream, codes, lengths, header, header_bits):
    """The deflate stream's bytes: the header's bits from bit 0, then every stream byte's code and the end-of-block code, each
    `lengths[s]` bits of the already bit-reversed `codes[s]` from bit 0, into bytes filled from the least significant bit; the last
    byte zero-padded."""
    sym = np.concatenate([np.asarray(stream).reshape(-1).astype(np.int64), [256]])
    ln = np.asarray(lengths, dtype=np.int64)[sym]
    cd = np.asarray(codes, dtype=np.int64)[sym]
    start = header_bits + np.cumsum(ln) - ln
    total = int(header_bits + ln.sum())
    bits = np.zeros(total, dtype=np.uint8)
    bits[:header_bits] = [(header >> j) & 1 for j in range(header_bits)]
    for j in range(15):
        m = ln > j
        bits[start[m] + j] = (cd[m] >> j) & 1
    return np.packbits(bits, bitorder='little').tobytes()
