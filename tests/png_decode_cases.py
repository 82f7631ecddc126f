"""TEST INFRASTRUCTURE for the PNG decoder (spaa_amd/png.py, csrc/png_decode.hip, csrc/png_inflate_core.hpp): PNG files and deflate
streams built by hand -- forced row filters, chosen zlib levels and strategies, fixed-Huffman and dynamic blocks written bit by
bit for what zlib never emits, and the malformed streams.  The CPU test runs every stream through the host build of the inflate
core under sanitizers; the GPU test decodes the same list.  Every well-formed hand-made stream is checked with zlib here."""
import functools
import struct
import zlib

import numpy as np

from spaa_amd import png

# SPAA_PNG_* of include/spaa_hip.h
OK, BAD_BLOCK_TYPE, STORED_LEN, OVERSUBSCRIBED, INCOMPLETE, BAD_REPEAT, BAD_SYMBOL, DIST_TOO_FAR, OUTPUT_LONG, INPUT_END, \
    OUTPUT_SHORT, BAD_FILTER, BAD_DESC = range(13)

CTYPE = {1: 0, 3: 2, 4: 6}


# ---- containers ---------------------------------------------------------------------------------------------------------------

def chunk(tag, body):
    return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body))


def make_png(w, h, channels, zstream, cuts=None, depth=8, ctype=None, interlace=0, extra=b''):
    """A PNG file around a zlib stream; `cuts`: byte positions at which the stream is split into IDAT chunks."""
    ihdr = struct.pack('>IIBBBBB', w, h, depth, CTYPE[channels] if ctype is None else ctype, 0, 0, interlace)
    edges = [0] + sorted(cuts or []) + [len(zstream)]
    idat = b''.join(chunk(b'IDAT', zstream[a:b]) for a, b in zip(edges, edges[1:]))
    return png.PNG_SIGNATURE + chunk(b'IHDR', ihdr) + extra + idat + chunk(b'IEND', b'')


def zwrap(deflate, raw):
    """zlib header + raw deflate + the Adler-32 of what it inflates to."""
    return b'\x78\x01' + deflate + struct.pack('>I', zlib.adler32(raw))


# ---- scanlines with forced filters ----------------------------------------------------------------------------------------------

def gradient_image(h, w, channels, seed=0):
    """Smooth gradient plus noise, uint8 [h, w, channels]: the Average and Paeth carries matter."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (3 * yy + 5 * xx)[..., None] + 40 * np.arange(channels)
    return ((base + rng.integers(0, 60, (h, w, channels))) % 256).astype(np.uint8)


def filter_rows(img, types):
    """The scanline stream of img [h, w, c] with filter types[y] forced on row y (PNG specification 9.2)."""
    h, w, c = img.shape
    x = img.reshape(h, w * c).astype(np.int32)
    a = np.zeros_like(x)
    a[:, c:] = x[:, :-c] if w > 1 else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    cc = np.zeros_like(x)
    cc[1:, c:] = x[:-1, :-c] if w > 1 else 0
    pa, pb, pc = abs(b - cc), abs(a - cc), abs(a + b - 2 * cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    pred = np.stack([np.zeros_like(x), a, b, (a + b) >> 1, paeth])
    t = np.asarray(types, dtype=np.int64)
    out = np.empty((h, 1 + w * c), np.uint8)
    out[:, 0] = t
    out[:, 1:] = (x - pred[t, np.arange(h)]) & 255
    return out.tobytes()


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None, every=500):
    """A zlib stream of raw; `flush`: that flush mode after every `every` input bytes."""
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    if flush is None:
        return co.compress(raw) + co.flush()
    out = b''
    for i in range(0, len(raw), every):
        out += co.compress(raw[i:i + every]) + co.flush(flush)
    return out + co.flush()


# ---- deflate by hand ----------------------------------------------------------------------------------------------------------------

class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, n):
        """n bits of value, least significant first (header fields, extra bits)."""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """A Huffman code of n bits, most significant first."""
        self.bits(int(format(code, f'0{n}b')[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def put_tokens(bw, tokens, lit_lens, dist_lens):
    """tokens: a literal byte, (length, distance), or ('sym', s) / ('dist', s) for a raw symbol; then the end of block."""
    lc, dc = png.canonical_codes(list(lit_lens)), png.canonical_codes(list(dist_lens)) if any(dist_lens) else []
    rev = [int(format(c, f'0{n}b')[::-1], 2) if n else 0 for c, n in zip(lc, lit_lens)]      # literals are most of the tokens
    for t in tokens:
        if isinstance(t, (int, np.integer)):
            bw.bits(rev[t], lit_lens[t])
        elif t[0] == 'sym':
            bw.code(lc[t[1]], lit_lens[t[1]])
        elif t[0] == 'dist':
            bw.code(dc[t[1]], dist_lens[t[1]])
        else:
            length, dist = t
            ls = max(s for s in range(29) if LBASE[s] <= length) if length < 258 else 28
            bw.code(lc[257 + ls], lit_lens[257 + ls])
            bw.bits(length - LBASE[ls], LEXT[ls])
            ds = max(s for s in range(30) if DBASE[s] <= dist)
            bw.code(dc[ds], dist_lens[ds])
            bw.bits(dist - DBASE[ds], DEXT[ds])
    bw.code(lc[256], lit_lens[256])


def fixed_block(bw, tokens, final=True):
    bw.bits(int(final), 1)
    bw.bits(1, 2)
    put_tokens(bw, tokens, FIXED_LIT, FIXED_DIST)


def stored_block(bw, data, final=True, nlen=None):
    bw.bits(int(final), 1)
    bw.bits(0, 2)
    bw.align()
    bw.bits(len(data), 16)
    bw.bits((~len(data) & 0xffff) if nlen is None else nlen, 16)
    for v in data:
        bw.bits(v, 8)


def rle_lens(lens):
    """Code-length symbols [(symbol, extra value)] for the CONCATENATED literal and distance lengths: runs cross the boundary."""
    seq, i = [], 0
    while i < len(lens):
        v, run = lens[i], 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            r = min(run, 138)
            seq.append((18, r - 11) if r >= 11 else (17, r - 3))
            i += r
        elif run >= 4:
            r = min(run - 1, 6)
            seq += [(v, 0), (16, r - 3)]
            i += 1 + r
        else:
            seq.append((v, 0))
            i += 1
    return seq


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}


def dynamic_header(bw, hlit, hdist, seq, final=True, cl_lens=None):
    """BFINAL, BTYPE = 2, HLIT, HDIST, HCLEN, the code-length code and the symbols `seq`; `cl_lens`: the 19 lengths of the
    code-length code by symbol (default: a Huffman code for seq)."""
    if cl_lens is None:
        counts = [0] * 19
        for s, _ in seq:
            counts[s] += 1
        if sum(c > 0 for c in counts) < 2:                 # a complete code needs two symbols
            counts[[k for k in range(19) if not counts[k]][0]] = 1
        cl_lens = png.huffman_lengths(counts, 7)
    codes = png.canonical_codes(list(cl_lens))
    bw.bits(int(final), 1)
    bw.bits(2, 2)
    bw.bits(hlit - 257, 5)
    bw.bits(hdist - 1, 5)
    bw.bits(19 - 4, 4)
    for s in CL_ORDER:
        bw.bits(cl_lens[s], 3)
    for s, extra in seq:
        bw.code(codes[s], cl_lens[s])
        if s >= 16:
            bw.bits(extra, CL_EXTRA[s])


def dynamic_block(bw, lit_lens, dist_lens, tokens, final=True):
    dynamic_header(bw, len(lit_lens), len(dist_lens), rle_lens(list(lit_lens) + list(dist_lens)), final)
    put_tokens(bw, tokens, lit_lens, dist_lens)


# ---- the stream list --------------------------------------------------------------------------------------------------------------

class Case:
    """One deflate payload: the image shape that announces its output size, the status the decoder must report and, when that is
    OK, the scanline bytes."""

    def __init__(self, name, payload, shape, status=OK, raw=None):
        self.name, self.payload, self.shape, self.status, self.raw = name, bytes(payload), shape, status, raw
        h, w, c = shape
        self.expect = h * (1 + w * c)
        if status == OK:
            assert raw is not None and len(raw) == self.expect, name
            assert zlib.decompress(self.payload, -15) == raw, name           # the oracle for scanline streams

    def record(self, adler=None):
        h, w, c = self.shape
        return png.PngRecord(w, h, c, self.payload, zlib.adler32(self.raw or b'') if adler is None else adler)

    def file(self):
        h, w, c = self.shape
        return make_png(w, h, c, zwrap(self.payload, self.raw))


def strip(z):
    return z[2:-4]


def _grey_row(n_bytes):
    """Shape of a one-row grey image whose scanline stream has n_bytes bytes (the first is the filter type)."""
    return (1, n_bytes - 1, 1)


HAND_SHAPE = (105, 105, 3)      # scanline stream 105 * 316 = 33180 bytes: the smallest square that holds 32768 + 258


def _hand_raw(seed):
    img = np.random.default_rng(seed).integers(0, 256, HAND_SHAPE, dtype=np.uint8)
    return bytearray(filter_rows(img, [0] * HAND_SHAPE[0]))


def hand_match(name, at, length, dist, seed=7):
    """A fixed-Huffman stream of the 105 x 105 image: literals, except ONE match (length, dist) at output position `at`."""
    raw = _hand_raw(seed)
    for i in range(length):
        raw[at + i] = raw[at + i - dist]
    row = 1 + 3 * HAND_SHAPE[1]
    assert all(raw[k] <= 4 for k in range(0, len(raw), row)), name        # the filter bytes stay filter types
    raw = bytes(raw)
    bw = BitWriter()
    fixed_block(bw, list(raw[:at]) + [(length, dist)] + list(raw[at + length:]))
    return Case(name, bw.bytes(), HAND_SHAPE, raw=raw)


RING, PIECE = 32768, 8192       # csrc/png_decode.hip: the history ring and the pieces it is flushed in


@functools.lru_cache(maxsize=None)
def hand_cases():
    row = 316
    return [
        hand_match('fixed_d32768_l258', 104 * row + 1, 258, 32768),
        hand_match('fixed_d1_l258', 50 * row + 20, 258, 1),
        hand_match('fixed_d3_l10', 3 * row + 100, 10, 3),
        hand_match('fixed_cross_flush', PIECE - 100, 258, row),          # the match spans output position 8192: a flush between
        hand_match('fixed_cross_ring', RING - 100, 258, row),            # ... and 32768: the ring wraps inside the copy
    ]


def _lens(n, pairs):
    out = [0] * n
    for s, b in pairs:
        out[s] = b
    return out


@functools.lru_cache(maxsize=None)
def block_cases():
    """Well-formed streams by hand for what zlib does not emit on request."""
    cases = []
    # code-length runs that cross from the literal/length table into the distance table: ..., [256] = 2, [257] = 2 | 2, 2, 2, 2
    lit, dist = _lens(258, [(0, 1), (256, 2), (257, 2)]), [2, 2, 2, 2]
    seq = rle_lens(lit + dist)
    assert seq[-2:] == [(2, 0), (16, 2)], seq                             # one 2, then "repeat 5 times": across the boundary
    raw = bytes(20 + 3 + 4)
    bw = BitWriter()
    dynamic_block(bw, lit, dist, [0] * 20 + [(3, 1)] + [0] * 4, final=True)
    cases.append(Case('dyn_run_crosses_tables', bw.bytes(), _grey_row(len(raw)), raw=raw))
    # code lengths 1 .. 15 (symbols 0 .. 14, and 256 with the second 15-bit code), no distance code in use
    lit = _lens(257, [(s, s + 1) for s in range(15)] + [(256, 15)])
    raw = bytes([0] + [s for s in range(15)] * 3 + [14, 13, 12, 11, 10, 9])
    bw = BitWriter()
    dynamic_block(bw, lit, [0], list(raw))
    cases.append(Case('dyn_lengths_to_15', bw.bytes(), _grey_row(len(raw)), raw=raw))
    # a single distance code of length 1, matches of distance 1 only
    lit = _lens(286, [(0, 2), (7, 2), (256, 2), (285, 2)])
    raw = bytes([0, 7]) + bytes([7]) * 258 + bytes([0]) + bytes([0]) * 258
    bw = BitWriter()
    dynamic_block(bw, lit, [1], [0, 7, (258, 1), 0, (258, 1)])
    cases.append(Case('dyn_single_distance_code', bw.bytes(), _grey_row(len(raw)), raw=raw))
    # stored blocks: empty ones, several in a row, then a fixed and a dynamic block in the same stream
    bw = BitWriter()
    stored_block(bw, b'', final=False)
    stored_block(bw, b'\x01abc', final=False)
    stored_block(bw, b'', final=False)
    stored_block(bw, b'', final=False)
    fixed_block(bw, list(b'defg') + [(6, 3)], final=False)
    dynamic_block(bw, _lens(257, [(120, 1), (256, 1)]), [0], [120] * 9, final=False)
    stored_block(bw, b'xyz', final=False)
    fixed_block(bw, [], final=True)
    raw = b'\x01abcdefgefgefg' + b'x' * 9 + b'xyz'
    cases.append(Case('mixed_blocks_empty_stored', bw.bytes(), _grey_row(len(raw)), raw=raw))
    return cases


@functools.lru_cache(maxsize=None)
def malformed_cases():
    """The streams that break one rule each, with the status that names it."""
    cases = []
    lits = bytes([0]) + bytes(range(150, 190))                       # 9-bit fixed codes: the cut falls inside a symbol
    bw = BitWriter()
    fixed_block(bw, list(lits))
    whole = bw.bytes()
    assert zlib.decompress(whole, -15) == lits
    cases.append(Case('truncated_mid_symbol', whole[:len(whole) // 2], _grey_row(len(lits)), INPUT_END))
    bw = BitWriter()
    stored_block(bw, bytes(40))
    cases.append(Case('truncated_mid_stored', bw.bytes()[:25], _grey_row(40), INPUT_END))
    cases.append(Case('truncated_stored_header', bw.bytes()[:3], _grey_row(40), INPUT_END))
    bw = BitWriter()
    stored_block(bw, bytes(40), nlen=0x1234)
    cases.append(Case('stored_len_nlen', bw.bytes(), _grey_row(40), STORED_LEN))
    bw = BitWriter()
    bw.bits(1, 1)
    bw.bits(3, 2)
    bw.bits(0, 29)
    cases.append(Case('block_type_3', bw.bytes(), _grey_row(40), BAD_BLOCK_TYPE))
    # over-subscribed: three code-length codes of one bit; and 257 literal codes of one bit
    bw = BitWriter()
    dynamic_header(bw, 257, 1, [(0, 0)] * 258, cl_lens=_lens(19, [(0, 1), (1, 1), (2, 1)]))
    cases.append(Case('oversubscribed_code_lengths', bw.bytes() + bytes(8), _grey_row(40), OVERSUBSCRIBED))
    bw = BitWriter()
    dynamic_header(bw, 257, 1, [(1, 0)] * 257 + [(0, 0)])
    cases.append(Case('oversubscribed_literals', bw.bytes() + bytes(8), _grey_row(40), OVERSUBSCRIBED))
    # incomplete: two literal codes of two bits
    bw = BitWriter()
    dynamic_header(bw, 257, 1, rle_lens(_lens(257, [(0, 2), (256, 2)]) + [0]))
    cases.append(Case('incomplete_literals', bw.bytes() + bytes(8), _grey_row(40), INCOMPLETE))
    # ... and two distance codes of two bits beside a complete literal code
    bw = BitWriter()
    dynamic_header(bw, 257, 2, rle_lens(_lens(257, [(0, 1), (256, 1)]) + [2, 2]))
    cases.append(Case('incomplete_distances', bw.bytes() + bytes(8), _grey_row(40), INCOMPLETE))
    bw = BitWriter()
    dynamic_header(bw, 257, 1, [(16, 0)] + [(0, 0)] * 255)
    cases.append(Case('repeat_16_first', bw.bytes() + bytes(8), _grey_row(40), BAD_REPEAT))
    bw = BitWriter()
    dynamic_header(bw, 257, 1, [(1, 0), (18, 127), (18, 127 - 11)])              # 1 + 138 + 127 = 266 > 257 + 1
    cases.append(Case('repeat_past_tables', bw.bytes() + bytes(8), _grey_row(40), BAD_REPEAT))
    bw = BitWriter()
    bw.bits(1, 1)
    bw.bits(1, 2)
    put_tokens(bw, [0, 9, (3, 3)], FIXED_LIT, FIXED_DIST)                         # two bytes out, distance 3
    cases.append(Case('distance_past_start', bw.bytes(), _grey_row(5), DIST_TOO_FAR))
    raw = bytes([0]) + bytes(range(30))
    good = strip(deflate(raw, 6))
    cases.append(Case('output_one_longer', good, _grey_row(len(raw) - 1), OUTPUT_LONG))
    cases.append(Case('output_one_shorter', good, _grey_row(len(raw) + 1), OUTPUT_SHORT))
    bw = BitWriter()
    fixed_block(bw, list(raw[:11]) + [(20, 5)])
    assert zlib.decompress(bw.bytes(), -15) == raw[:11] + (raw[6:11] * 4)
    cases.append(Case('match_one_longer', bw.bytes(), _grey_row(30), OUTPUT_LONG))
    cases.append(Case('empty_payload', b'', _grey_row(40), INPUT_END))
    bw = BitWriter()
    bw.bits(1, 1)
    bw.bits(1, 2)
    put_tokens(bw, [0, ('sym', 286)], FIXED_LIT, FIXED_DIST)
    cases.append(Case('symbol_286', bw.bytes(), _grey_row(40), BAD_SYMBOL))
    bw = BitWriter()
    bw.bits(1, 1)
    bw.bits(1, 2)
    put_tokens(bw, [0, 0, ('sym', 257), ('dist', 30)], FIXED_LIT, FIXED_DIST)
    cases.append(Case('distance_code_30', bw.bytes(), _grey_row(40), BAD_SYMBOL))
    return cases


def zlib_cases():
    """The block kinds zlib emits: (name, shape, zlib stream, scanlines)."""
    img = gradient_image(33, 40, 3)
    raw = filter_rows(img, [y % 5 for y in range(33)])
    out = [('level1', deflate(raw, 1)), ('level9', deflate(raw, 9)), ('fixed', deflate(raw, 6, zlib.Z_FIXED)),
           ('huffman_only', deflate(raw, 6, zlib.Z_HUFFMAN_ONLY)), ('rle', deflate(raw, 6, zlib.Z_RLE)),
           ('sync_flush', deflate(raw, 6, flush=zlib.Z_SYNC_FLUSH)), ('full_flush', deflate(raw, 6, flush=zlib.Z_FULL_FLUSH))]
    cases = [Case('zlib_' + n, strip(z), (33, 40, 3), raw=raw) for n, z in out]
    big = gradient_image(150, 150, 3, seed=3)
    raw0 = filter_rows(big, [0] * 150)
    assert len(raw0) > 65535
    cases.append(Case('zlib_level0_two_stored', strip(deflate(raw0, 0)), (150, 150, 3), raw=raw0))
    return cases


def filter_cases():
    """Each filter type on every row, and the five in turn, at 1x1, 7x1, 3x5 and 70x67, with 1, 3 and 4 channels."""
    cases = []
    for h, w in ((1, 1), (7, 1), (3, 5), (70, 67)):
        for c in (1, 3, 4):
            img = gradient_image(h, w, c)
            for kind in (0, 1, 2, 3, 4, 'cycle'):
                types = [y % 5 for y in range(h)] if kind == 'cycle' else [kind] * h
                raw = filter_rows(img, types)
                cases.append(Case(f'filter_{kind}_{h}x{w}x{c}', strip(deflate(raw, 6)), (h, w, c), raw=raw))
    return cases


def filter5_case():
    """Scanlines that inflate well and whose first row names filter type 5: the unfilter step must report it."""
    raw = bytearray(filter_rows(gradient_image(3, 5, 3), [0, 1, 2]))
    raw[0] = 5
    return Case('filter_byte_5', strip(deflate(bytes(raw), 6)), (3, 5, 3), raw=bytes(raw))


def all_inflate_cases():
    """Every stream the GPU tests decode, well-formed and malformed: the host program sees all of them first."""
    return filter_cases() + zlib_cases() + block_cases() + hand_cases() + [filter5_case()] + malformed_cases()


def write_container(path, cases):
    """The input of tests/host/png_inflate_host.cpp."""
    with open(path, 'wb') as fh:
        fh.write(b'PIS1' + struct.pack('<I', len(cases)))
        for c in cases:
            ref = c.raw if c.status == OK else b''
            fh.write(struct.pack('<IIII', len(c.payload), c.expect, c.status, len(ref)) + c.payload + ref)
