"""PNG encoding and decoding of device-resident images: the host half (pure Python / numpy; importing it needs no GPU), `encode_png`,
which drives the two entry points of csrc/png.hip, and `decode_png`, which drives the two of csrc/png_decode.hip.

The scheme: per row the cheapest of the five PNG filters, then ONE dynamic-Huffman deflate block of literals
only -- no LZ77 matching.  The device filters the images, counts the bytes and packs the bits; the host builds, per image, a
length-limited Huffman code from the 257 counts (`huffman_lengths`), the block header (`deflate_tables`) and the PNG container
(`wrap_png`).  Because the code lengths are known before the bits are packed, every image's stream size is exact before the
second launch.

Decoding ("The read side"): the host walks the chunks, checks their CRCs and the zlib header (`parse_png`) and packs
the raw deflate payloads of a batch into one pinned buffer; the device inflates them, one wave per image, and undoes the row
filters; the Adler-32 of every image's scanlines comes back as per-row sums and is compared with the stream's trailer.
"""
import collections
import heapq
import struct
import zlib

import numpy as np

PACK_RUN, PACK_CHUNK = 16, 4096      # csrc/png.hip: symbols per thread and per workgroup of the packer
HDR_WORDS = 64                       # block header: at most 2048 bits
MAX_ROW_BYTES = 30000                # 3 W: the filter kernel stages two rows in LDS
ADLER_MOD = 65521
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def _rev16_table():
    v = np.arange(1 << 16, dtype=np.uint32)
    for sh, mask in ((1, 0x5555), (2, 0x3333), (4, 0x0f0f), (8, 0x00ff)):
        v = (v >> sh & mask) | (v & mask) << sh
    return v


_REV16 = _rev16_table()              # 16-bit bit reversal


def huffman_lengths(counts, max_bits):
    """Code lengths (list of int, 0 for unused symbols) of a length-limited prefix code for `counts`: a Huffman code when its
    tree is at most `max_bits` deep; otherwise the lengths are capped and the over-subscribed code is repaired one unit of the
    Kraft sum at a time (a code of the longest length is dropped beside a shorter one that moves one level down), and the
    lengths are handed out again by frequency.  With two or more used symbols the code is complete (Kraft sum exactly 1), as
    zlib demands of a literal or code-length code; a single used symbol gets length 1."""
    counts = [int(c) for c in counts]
    used = [i for i, c in enumerate(counts) if c > 0]
    lengths = [0] * len(counts)
    if len(used) < 2:
        for i in used:
            lengths[i] = 1
        return lengths
    if (1 << max_bits) < len(used):
        raise ValueError(f'huffman_lengths: {len(used)} symbols do not fit {max_bits} bits')
    # Huffman: parent links, then each leaf's depth (nodes are created in order: a parent has a larger index than its children)
    heap = [(counts[s], k) for k, s in enumerate(used)]
    heapq.heapify(heap)
    parent = [0] * (2 * len(used) - 1)
    nxt = len(used)
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        parent[a[1]] = parent[b[1]] = nxt
        heapq.heappush(heap, (a[0] + b[0], nxt))
        nxt += 1
    depth = [0] * len(parent)
    for k in range(len(parent) - 2, -1, -1):
        depth[k] = depth[parent[k]] + 1
    leaf = depth[:len(used)]
    if max(leaf) <= max_bits:
        for k, s in enumerate(used):
            lengths[s] = leaf[k]
        return lengths
    num = [0] * (max_bits + 1)                       # codes per length, depths beyond the limit capped to it
    for d in leaf:
        num[min(d, max_bits)] += 1
    total = sum(num[b] << (max_bits - b) for b in range(1, max_bits + 1))
    while total > (1 << max_bits):
        num[max_bits] -= 1
        for b in range(max_bits - 1, 0, -1):
            if num[b]:
                num[b] -= 1
                num[b + 1] += 2
                break
        total -= 1
    order = sorted(used, key=lambda s: (-counts[s], s))      # most frequent first: the shortest codes
    k = 0
    for b in range(1, max_bits + 1):
        for s in order[k:k + num[b]]:
            lengths[s] = b
        k += num[b]
    return lengths


def canonical_codes(lengths):
    """Canonical Huffman codes (RFC 1951 3.2.2) of `lengths`, most significant bit first; 0 for unused symbols."""
    max_bits = max(lengths)
    bl = [0] * (max_bits + 2)
    for b in lengths:
        if b:
            bl[b] += 1
    code, nxt = 0, [0] * (max_bits + 2)
    for b in range(1, max_bits + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lengths)
    for i, b in enumerate(lengths):
        if b:
            out[i] = nxt[b]
            nxt[b] += 1
    return out


def _reversed(code, nbits):
    return int(_REV16[code]) >> (16 - nbits) if nbits else 0


def deflate_tables(hist):
    """One deflate block for an image whose stream has the byte counts hist[0..255] (hist[256], the end of block, counts once):
    -> (codes, lengths, header, header_bits).  codes uint32 [257]: the canonical literal codes, BIT-REVERSED so that they can
    be ORed into a stream that fills bytes from the least significant bit; lengths uint8 [257] (<= 15, 0 = unused); header: a
    Python int holding the header's bits from bit 0 -- BFINAL = 1, BTYPE = 2, HLIT = 257, HDIST = 1, HCLEN, the code-length
    code's lengths (<= 7 bits), then the 257 literal lengths and the one distance length 0, each as its own code-length symbol
    (no repeat symbols 16 / 17 / 18: they would save a few dozen bytes per image)."""
    hist = [int(c) for c in np.asarray(hist).reshape(-1)]
    if len(hist) != 257:
        raise ValueError(f'deflate_tables: expected 257 counts, got {len(hist)}')
    hist[256] = 1
    lit = huffman_lengths(hist, 15)
    seq = lit + [0]                                   # + the single distance code, length 0 (never used: no matches)
    cl_counts = [0] * 19
    for b in seq:
        cl_counts[b] += 1
    cl = huffman_lengths(cl_counts, 7)
    cl_rev = [_reversed(c, b) for c, b in zip(canonical_codes(cl), cl)]
    hclen = 19
    while hclen > 4 and cl[_CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    acc, n = 1 | 2 << 1 | 0 << 3 | 0 << 8 | (hclen - 4) << 13, 17          # BFINAL, BTYPE, HLIT - 257, HDIST - 1, HCLEN - 4
    for i in range(hclen):
        acc |= cl[_CL_ORDER[i]] << n
        n += 3
    for b in seq:
        acc |= cl_rev[b] << n
        n += cl[b]
    lengths = np.array(lit, dtype=np.uint8)
    codes = _REV16[np.array(canonical_codes(lit), dtype=np.int64)] >> (16 - lengths.astype(np.uint32))
    codes = np.where(lengths > 0, codes, 0).astype(np.uint32)
    return codes, lengths, acc, n


def deflate_bits(hist, lengths, header_bits):
    """Exact length in bits of the block: header, every stream byte's code, the end of block."""
    h = np.asarray(hist, dtype=np.int64).copy()
    h[256] = 1
    return int(header_bits + (h * np.asarray(lengths, dtype=np.int64)).sum())


def adler32_from_rows(row_sums, row_len):
    """Adler-32 of a stream of rows of `row_len` bytes from the per-row partial sums [..., H, 2] = (sum of the row's bytes, sum of
    byte j times (row_len - j)), plain or mod 65521.  Vectorised over leading axes; returns uint32 [...]."""
    r = np.asarray(row_sums).astype(np.int64) % ADLER_MOD
    s1, s2 = r[..., 0], r[..., 1]
    a_before = (1 + np.cumsum(s1, axis=-1) - s1) % ADLER_MOD       # `a` when the row starts
    a = (1 + s1.sum(axis=-1)) % ADLER_MOD
    b = (((row_len % ADLER_MOD) * a_before) % ADLER_MOD + s2).sum(axis=-1) % ADLER_MOD
    return (b << 16 | a).astype(np.uint32)


def _chunk(tag, body):
    return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body))


def wrap_png(width, height, deflate_bytes, adler32):
    """The PNG file around one raw deflate stream of the scanlines: signature, IHDR (8 bits, colour type 2 = RGB, no interlace),
    one IDAT holding the zlib stream (header 78 01, the deflate bytes, the big-endian Adler-32 of the scanline stream), IEND."""
    ihdr = struct.pack('>IIBBBBB', int(width), int(height), 8, 2, 0, 0, 0)
    idat = b'\x78\x01' + bytes(deflate_bytes) + struct.pack('>I', int(adler32))
    return b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', idat) + _chunk(b'IEND', b'')


def _check_images(images):
    import torch
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise RuntimeError('spaa_amd.png encodes on the GPU only (no CPU fallback): images is '
                           f'{"on " + str(images.device) if isinstance(images, torch.Tensor) else type(images).__name__}')
    if images.ndim != 4 or images.shape[1] != 3 or images.dtype not in (torch.float32, torch.uint8) or 0 in images.shape:
        raise ValueError(f'encode_png: expected float32 or uint8 [N,3,H,W], got {images.dtype} {tuple(images.shape)}')
    if 3 * images.shape[3] > MAX_ROW_BYTES:
        raise ValueError(f'encode_png: images at most {MAX_ROW_BYTES // 3} wide, got {images.shape[3]}')
    return images.detach().contiguous()


def filter_hist(images):
    """spaa_png_filter_hist on float32 / uint8 CUDA images [N,3,H,W] -> (streams uint8 [N, H (1 + 3 W)], stats int32
    [N 257 + N H 2]) on the device; stats holds the histograms [N,257], then the Adler row sums [N,H,2]."""
    import torch
    from . import _lib
    x = _check_images(images)
    n, _, h, w = x.shape
    with _lib.on_device(x.device):
        streams = torch.empty(n, h * (1 + 3 * w), dtype=torch.uint8, device=x.device)
        stats = torch.empty(n * 257 + n * h * 2, dtype=torch.int32, device=x.device)
        _lib.call('spaa_png_filter_hist', _lib.ptr(x), int(x.dtype == torch.float32), n, h, w, _lib.ptr(streams),
                  _lib.ptr(stats), _lib.ptr(stats[n * 257:]))
    return streams, stats


def pack(streams, codes, lengths, headers, header_bits, offsets, out_bytes):
    """spaa_png_pack: streams uint8 [N,S] on the device; per image codes / lengths [N,257], header ints and their bit counts,
    byte offsets into the ragged buffer of `out_bytes` bytes (rounded up to a multiple of 4 here).  Returns the uint8 buffer on
    the device."""
    import torch
    from . import _lib
    n, s = streams.shape
    nchunk = s // PACK_CHUNK + 1
    # one host block, one copy: tables [N,257] u32 | header words [N,64] u32 | header bit counts [N] i32 (+ pad) | offsets [N] i64
    words = n * 257 + n * HDR_WORDS + n                  # (even: the offsets that follow are 8-byte aligned)
    meta = np.zeros(words + 2 * n, dtype=np.uint32)
    meta[:n * 257] = (np.asarray(codes, dtype=np.uint32) | np.asarray(lengths, dtype=np.uint32) << 16).reshape(-1)
    hdr = meta[n * 257:n * 257 + n * HDR_WORDS].reshape(n, HDR_WORDS)
    for i, (v, nb) in enumerate(zip(headers, header_bits)):
        if nb > 32 * HDR_WORDS:
            raise ValueError(f'pack: a block header of {nb} bits')
        hdr[i] = np.frombuffer(int(v).to_bytes(4 * HDR_WORDS, 'little'), dtype='<u4')
    o = n * 257 + n * HDR_WORDS
    meta[o:o + n] = np.asarray(header_bits, dtype=np.uint32)
    meta[words:].view(np.int64)[:] = np.asarray(offsets, dtype=np.int64)
    out_bytes = (int(out_bytes) + 3) & ~3
    dev = streams.device
    with _lib.on_device(dev):
        meta_d = torch.from_numpy(meta.view(np.int32)).to(dev)
        scratch = torch.empty(n * nchunk, dtype=torch.int32, device=dev)
        out = torch.zeros(max(out_bytes, 4), dtype=torch.uint8, device=dev)
        _lib.call('spaa_png_pack', _lib.ptr(streams), s, n, _lib.ptr(meta_d), _lib.ptr(meta_d[n * 257:]), _lib.ptr(meta_d[o:]),
                  _lib.ptr(meta_d[words:]), _lib.ptr(scratch), _lib.ptr(out), out.numel())
    return out


MAX_STREAM_BYTES = 1 << 28      # scanline bytes per pair of launches: larger batches are encoded in pieces


def encode_png(images, timings=None):
    """PNG files (a list of `bytes`) of float32 or uint8 CUDA images [N,3,H,W].  A float x is written as the low 8 bits of
    (int32)(x * 255) in fp32 -- np.uint8(x * 255) for x in [0, 1], truncation; values outside [0, 1] get those low 8 bits, NaN
    and inf are unspecified.  Per batch: the filter launch, one copy of the histograms and Adler sums to the host, the Huffman
    tables, the pack launch, one copy of the ragged deflate buffer, the containers.  A CPU tensor or a missing library raises.
    `timings`: a dict that receives the seconds spent in 'filter', 'tables', 'pack', 'wrap' (each ends in a synchronising copy)."""
    import time
    x = _check_images(images)
    n, _, h, w = x.shape
    row = 1 + 3 * w
    per = max(1, min(65535, MAX_STREAM_BYTES // (h * row)))
    files = []
    t = dict(filter=0.0, tables=0.0, pack=0.0, wrap=0.0)
    for a in range(0, n, per):
        xs = x[a:a + per]
        m = xs.shape[0]
        t0 = time.perf_counter()
        streams, stats = filter_hist(xs)
        stats = stats.cpu().numpy()
        t1 = time.perf_counter()
        hist = stats[:m * 257].reshape(m, 257)
        adler = adler32_from_rows(stats[m * 257:].reshape(m, h, 2), row)
        tabs = [deflate_tables(hist[i]) for i in range(m)]
        nbytes = [(deflate_bits(hist[i], tb[1], tb[3]) + 7) // 8 for i, tb in enumerate(tabs)]
        offsets = np.concatenate(([0], np.cumsum(nbytes)))
        t2 = time.perf_counter()
        out = pack(streams, np.stack([tb[0] for tb in tabs]), np.stack([tb[1] for tb in tabs]), [tb[2] for tb in tabs],
                   [tb[3] for tb in tabs], offsets[:-1], offsets[-1]).cpu().numpy()
        t3 = time.perf_counter()
        buf = out.tobytes()
        files += [wrap_png(w, h, buf[offsets[i]:offsets[i + 1]], adler[i]) for i in range(m)]
        t4 = time.perf_counter()
        for k, v in zip(('filter', 'tables', 'pack', 'wrap'), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            t[k] += v
    if timings is not None:
        timings.update(t)
    return files


# ---- the read side -------------------------------------------------------------------------------------------------------------

PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'
MAX_DECODE_WIDTH = 16000             # csrc/png_decode.hip: the unfilter kernel keeps one row of packed pixels in LDS
ST_ADLER = 100                       # host-side status: the scanlines' Adler-32 is not the stream's trailer
STATUS_TEXT = {                      # include/spaa_hip.h, SPAA_PNG_*
    1: 'reserved deflate block type 3',
    2: 'stored block whose LEN and NLEN do not match',
    3: 'over-subscribed Huffman code set',
    4: 'incomplete Huffman code set',
    5: 'code-length repeat with nothing to repeat or past the end of the table',
    6: 'invalid literal/length or distance symbol',
    7: 'match distance beyond the start of the output',
    8: 'more scanline data than the header announces',
    9: 'deflate stream ends early',
    10: 'less scanline data than the header announces',
    11: 'scanline filter type above 4',
    12: 'image descriptor out of range',
    ST_ADLER: 'Adler-32 of the scanlines does not match the stream trailer',
}

PngRecord = collections.namedtuple('PngRecord', 'width height channels deflate adler')
PngRecord.__doc__ = """What the device needs of one PNG file: size, channels (1, 3 or 4), the raw deflate payload of the concatenated
IDAT chunks (zlib header and trailer stripped) and the trailer's Adler-32."""


def parse_png(data):
    """The container of one PNG file -> PngRecord, or None for a well-formed file the device path does not take (palette, 16-bit,
    1/2/4-bit, interlaced, wider than MAX_DECODE_WIDTH: read those with Pillow).  Checks the signature, every chunk's CRC, IHDR
    first, at least one IDAT, IEND, and the zlib header (deflate, window <= 32 KiB, FCHECK, no preset dictionary); ancillary chunks
    are skipped.  A broken container raises ValueError."""
    data = bytes(data)
    if data[:8] != PNG_SIGNATURE:
        raise ValueError('not a PNG file: bad signature')
    i, hdr, idat, seen_idat, ended = 8, None, [], False, False
    while i < len(data):
        if i + 12 > len(data):
            raise ValueError('truncated chunk header')
        n = int.from_bytes(data[i:i + 4], 'big')
        tag = data[i + 4:i + 8]
        if i + 12 + n > len(data):
            raise ValueError(f'chunk {tag!r} runs past the end of the file')
        body = data[i + 8:i + 8 + n]
        if zlib.crc32(data[i + 4:i + 8 + n]) != int.from_bytes(data[i + 8 + n:i + 12 + n], 'big'):
            raise ValueError(f'chunk {tag!r}: bad CRC')
        i += 12 + n
        if hdr is None and tag != b'IHDR':
            raise ValueError('missing IHDR: the first chunk is ' + repr(tag))
        if tag == b'IHDR':
            if hdr is not None or n != 13:
                raise ValueError('bad IHDR')
            hdr = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat.append(body)
            seen_idat = True
        elif tag == b'IEND':
            ended = True
            break
        elif not tag[0] & 0x20 and tag != b'PLTE':
            raise ValueError(f'unknown critical chunk {tag!r}')
    if hdr is None:
        raise ValueError('missing IHDR')
    if not seen_idat:
        raise ValueError('missing IDAT')
    if not ended:
        raise ValueError('missing IEND')
    w, h, depth, ctype, comp, filt, interlace = hdr
    if w == 0 or h == 0:
        raise ValueError(f'zero dimension: {w} x {h}')
    if depth not in (1, 2, 4, 8, 16) or ctype not in (0, 2, 3, 4, 6) or comp != 0 or filt != 0 or interlace not in (0, 1):
        raise ValueError(f'bad IHDR fields: depth {depth}, colour type {ctype}, compression {comp}, filter {filt}, interlace {interlace}')
    if depth != 8 or interlace != 0 or ctype not in (0, 2, 6) or w > MAX_DECODE_WIDTH or h * (1 + 4 * w) >= 1 << 31:
        return None
    z = b''.join(idat)
    if len(z) < 6:
        raise ValueError('IDAT: no room for a zlib header and trailer')
    cmf, flg = z[0], z[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf << 8 | flg) % 31 or flg & 0x20:
        raise ValueError(f'IDAT: bad zlib header {cmf:02x} {flg:02x}')
    return PngRecord(w, h, {0: 1, 2: 3, 6: 4}[ctype], z[2:-4], int.from_bytes(z[-4:], 'big'))


def _pin(t):
    try:
        return t.pin_memory()
    except RuntimeError:         # (no pinned allocation available: the copy is then staged by the runtime)
        return t


def decode_records(records, device, timings=None):
    """The device half of `decode_png` for PngRecords: -> (list of uint8 CUDA tensors [3,H,W], status int array [N]).  One pinned
    host block (descriptors, then every deflate payload on a 4-byte boundary), one copy to the device, spaa_png_inflate,
    spaa_png_unfilter, one copy back (the status words and the Adler row sums); status is 0, a SPAA_PNG_* code of
    include/spaa_hip.h, or ST_ADLER.  Images with a non-zero status hold unspecified bytes.  `timings`: a dict that receives
    the milliseconds of 'h2d', 'inflate', 'unfilter', 'd2h' measured with events on the stream."""
    import ctypes
    import torch
    from . import _lib
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError(f'spaa_amd.png decodes on the GPU only (no CPU fallback): device is {device}')
    n = len(records)
    if n == 0:
        return [], np.zeros(0, np.int32)
    descs = (_lib.PngImg * n)()
    dbytes = (ctypes.sizeof(descs) + 15) & ~15
    src, ws, out, row = dbytes, 0, 0, 0
    for d, r in zip(descs, records):
        d.src_off, d.src_len, d.H, d.W, d.channels = src - dbytes, len(r.deflate), r.height, r.width, r.channels
        d.ws_off, d.out_off, d.row0 = ws, out, row
        src += (len(r.deflate) + 3) & ~3
        ws += (r.height * (1 + r.width * r.channels) + 15) & ~15
        out += 3 * r.height * r.width
        row += r.height
    host = torch.empty(max(src, dbytes + 4), dtype=torch.uint8)
    host = _pin(host)
    hv = host.numpy()
    hv[:ctypes.sizeof(descs)] = np.frombuffer(descs, dtype=np.uint8)
    for d, r in zip(descs, records):
        hv[dbytes + d.src_off:dbytes + d.src_off + d.src_len] = np.frombuffer(r.deflate, dtype=np.uint8)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if timings is not None else None
    with _lib.on_device(device):
        if ev:
            ev[0].record()
        dev = host.to(device, non_blocking=True)
        work = torch.empty(ws, dtype=torch.uint8, device=device)
        pixels = torch.empty(out, dtype=torch.uint8, device=device)
        back = torch.empty(n + 2 * row, dtype=torch.int32, device=device)         # status [N] | Adler row sums [rows][2]
        if ev:
            ev[1].record()
        _lib.call('spaa_png_inflate', _lib.ptr(dev[dbytes:]), src - dbytes, _lib.ptr(dev), n, _lib.ptr(work), ws, _lib.ptr(back))
        if ev:
            ev[2].record()
        _lib.call('spaa_png_unfilter', _lib.ptr(work), ws, _lib.ptr(dev), n, max(r.width for r in records), _lib.ptr(pixels), out,
                  _lib.ptr(back[n:]), row, _lib.ptr(back))
        if ev:
            ev[3].record()
        back_h = back.cpu().numpy()
        if ev:
            ev[4].record()
            ev[4].synchronize()
            for k, name in enumerate(('h2d', 'inflate', 'unfilter', 'd2h')):
                timings[name] = ev[k].elapsed_time(ev[k + 1])
    status = back_h[:n].copy()
    sums = back_h[n:].view(np.uint32).reshape(row, 2)
    images = []
    for i, (d, r) in enumerate(zip(descs, records)):
        images.append(pixels[d.out_off:d.out_off + 3 * r.height * r.width].view(3, r.height, r.width))
        if status[i] == 0 and int(adler32_from_rows(sums[d.row0:d.row0 + r.height], 1 + r.width * r.channels)) != r.adler:
            status[i] = ST_ADLER
    return images, status


def decode_png(blobs, device, *, names=None):
    """PNG files (`bytes`) -> a list of uint8 CUDA tensors [3,H,W] on `device`, the pixels of `Image.open(...).convert('RGB')`: grey
    is replicated, alpha dropped.  The files of one call may differ in size and colour type; each must be one `parse_png`
    accepts (8-bit grey / RGB / RGBA, not interlaced).  One host-to-device copy and two launches whatever the number of files.
    A broken container, a deflate stream that breaks a rule, a bad filter type or an Adler-32 mismatch raises ValueError naming
    the file (`names[i]`, else its index) and the reason; nothing falls back to another decoder."""
    label = (lambda i: str(names[i])) if names is not None else (lambda i: f'image {i}')
    records = []
    for i, b in enumerate(blobs):
        try:
            r = parse_png(b)
        except ValueError as e:
            raise ValueError(f'decode_png: {label(i)}: {e}') from None
        if r is None:
            raise ValueError(f'decode_png: {label(i)}: not an 8-bit non-interlaced grey / RGB / RGBA file (parse_png declines it)')
        records.append(r)
    images, status = decode_records(records, device)
    bad = [f'{label(i)}: {STATUS_TEXT.get(int(s), "status " + str(int(s)))}' for i, s in enumerate(status) if s]
    if bad:
        raise ValueError('decode_png: ' + '; '.join(bad))
    return images
