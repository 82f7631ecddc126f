"""Result montages of the summary step on the GPU (HIP kernels, no CPU fallback): the reference's `attack_results`
(projector_based_attack.py:362-414), i.e. the SPAA paper's Figs. 4-5 -- for every attack five tiles (camera-captured scene,
adversarial projection, inferred capture, real capture, pseudo-colour difference of the last and the first) under two lines of text.

The reference builds one montage per attack on the host (three F.interpolate calls, a min / max pass, a numpy round trip, cv2's
colour map, torchvision's make_grid and seven PIL round trips for the text).  Here every montage of a setup is made from
device-resident images as final 8-bit pixels by two entry points of libspaa_hip.so (csrc/montage.hip), four kernels whatever the
number of montages:
  spaa_montage_diff_range   per montage, min and max of |rz(real) - rz(scene)|  (rz = centre crop + area resize)
  spaa_montage_compose      background, tiles, colour map, then the text from a list of glyph records
The arithmetic is specified to the fp32 operation (include/spaa_hip.h, DESIGN.md "Result montages"), so tests/montage_oracle.py --
the reference's own torch / numpy calls on the CPU -- reproduces the bytes exactly.  Neither cv2, torchvision nor PIL is needed.

Differences from the reference, all of the text and the colour table:
  * the text is a 1-bit bitmap font drawn for this project (FONT), not PIL's TrueType rendering of Arial at 14 pt;
  * labels sit at their tile's edges (`layout_labels`); the reference's hand-tuned x offsets for 256-pixel tiles are not kept;
  * JET restates the Jet colour map from its piecewise-linear definition; it has not been checked against OpenCV's table.  Any
    uint8 [256,3] RGB table can be passed as `colormap`.
"""
import numpy as np
import torch

from . import _lib
from .metrics import center_crop_origin

BAND, PAD = 26, 5            # text band above the grid; make_grid's padding
FONT_W, FONT_H = 6, 12       # glyph cell; two lines fit the band (2 * FONT_H <= BAND)
LINE1 = ('Cam-captured scene ({t})', 'Model inferred adversarial projection', 'Model inferred cam-captured projection',
         'Real cam-captured projection', 'Normalized difference, i.e., 4th-1st')

# The font: 5 x 7 dots per glyph ('#' = ink), two more rows for the descenders of g j p q y; rows separated by '/'.  Drawn by hand
# for this project.  A glyph sits in columns 0..4 and rows 1..9 of its FONT_W x FONT_H cell.
_GLYPHS = {
    ' ': '...../...../...../...../...../...../.....',
    '!': '..#../..#../..#../..#../..#../...../..#..',
    '"': '.#.#./.#.#./...../...../...../...../.....',
    '#': '.#.#./.#.#./#####/.#.#./#####/.#.#./.#.#.',
    '$': '..#../.####/#.#../.###./..#.#/####./..#..',
    '%': '##..#/##.#./...#./..#../.#.../.#.##/#..##',
    '&': '.##../#..#./#.#../.#.../#.#.#/#..#./.##.#',
    "'": '..#../..#../...../...../...../...../.....',
    '(': '...#./..#../.#.../.#.../.#.../..#../...#.',
    ')': '.#.../..#../...#./...#./...#./..#../.#...',
    '*': '...../..#../#.#.#/.###./#.#.#/..#../.....',
    '+': '...../..#../..#../#####/..#../..#../.....',
    ',': '...../...../...../...../..##./..#../.#...',
    '-': '...../...../...../#####/...../...../.....',
    '.': '...../...../...../...../...../.##../.##..',
    '/': '....#/...#./...#./..#../.#.../.#.../#....',
    '0': '.###./#...#/#..##/#.#.#/##..#/#...#/.###.',
    '1': '..#../.##../..#../..#../..#../..#../.###.',
    '2': '.###./#...#/....#/...#./..#../.#.../#####',
    '3': '####./....#/....#/.###./....#/....#/####.',
    '4': '...#./..##./.#.#./#..#./#####/...#./...#.',
    '5': '#####/#..../####./....#/....#/#...#/.###.',
    '6': '..##./.#.../#..../####./#...#/#...#/.###.',
    '7': '#####/....#/...#./..#../..#../.#.../.#...',
    '8': '.###./#...#/#...#/.###./#...#/#...#/.###.',
    '9': '.###./#...#/#...#/.####/....#/...#./.##..',
    ':': '...../.##../.##../...../.##../.##../.....',
    ';': '...../.##../.##../...../.##../..#../.#...',
    '<': '...#./..#../.#.../#..../.#.../..#../...#.',
    '=': '...../...../#####/...../#####/...../.....',
    '>': '.#.../..#../...#./....#/...#./..#../.#...',
    '?': '.###./#...#/....#/...#./..#../...../..#..',
    '@': '.###./#...#/#.###/#.#.#/#.###/#..../.####',
    'A': '..#../.#.#./#...#/#...#/#####/#...#/#...#',
    'B': '####./#...#/#...#/####./#...#/#...#/####.',
    'C': '.###./#...#/#..../#..../#..../#...#/.###.',
    'D': '###../#..#./#...#/#...#/#...#/#..#./###..',
    'E': '#####/#..../#..../####./#..../#..../#####',
    'F': '#####/#..../#..../####./#..../#..../#....',
    'G': '.###./#...#/#..../#.###/#...#/#...#/.####',
    'H': '#...#/#...#/#...#/#####/#...#/#...#/#...#',
    'I': '.###./..#../..#../..#../..#../..#../.###.',
    'J': '..###/...#./...#./...#./...#./#..#./.##..',
    'K': '#...#/#..#./#.#../##.../#.#../#..#./#...#',
    'L': '#..../#..../#..../#..../#..../#..../#####',
    'M': '#...#/##.##/#.#.#/#.#.#/#...#/#...#/#...#',
    'N': '#...#/##..#/#.#.#/#..##/#...#/#...#/#...#',
    'O': '.###./#...#/#...#/#...#/#...#/#...#/.###.',
    'P': '####./#...#/#...#/####./#..../#..../#....',
    'Q': '.###./#...#/#...#/#...#/#.#.#/#..#./.##.#',
    'R': '####./#...#/#...#/####./#.#../#..#./#...#',
    'S': '.####/#..../#..../.###./....#/....#/####.',
    'T': '#####/..#../..#../..#../..#../..#../..#..',
    'U': '#...#/#...#/#...#/#...#/#...#/#...#/.###.',
    'V': '#...#/#...#/#...#/#...#/.#.#./.#.#./..#..',
    'W': '#...#/#...#/#...#/#.#.#/#.#.#/##.##/#...#',
    'X': '#...#/#...#/.#.#./..#../.#.#./#...#/#...#',
    'Y': '#...#/#...#/.#.#./..#../..#../..#../..#..',
    'Z': '#####/....#/...#./..#../.#.../#..../#####',
    '[': '.###./.#.../.#.../.#.../.#.../.#.../.###.',
    '\\': '#..../.#.../.#.../..#../...#./...#./....#',
    ']': '.###./...#./...#./...#./...#./...#./.###.',
    '^': '..#../.#.#./#...#/...../...../...../.....',
    '_': '...../...../...../...../...../...../#####',
    '`': '.#.../..#../...../...../...../...../.....',
    'a': '...../...../.###./....#/.####/#...#/.####',
    'b': '#..../#..../#.##./##..#/#...#/#...#/####.',
    'c': '...../...../.###./#..../#..../#...#/.###.',
    'd': '....#/....#/.##.#/#..##/#...#/#...#/.####',
    'e': '...../...../.###./#...#/#####/#..../.###.',
    'f': '..##./.#..#/.#.../###../.#.../.#.../.#...',
    'g': '...../...../.####/#...#/#...#/#...#/.####/....#/.###.',
    'h': '#..../#..../#.##./##..#/#...#/#...#/#...#',
    'i': '..#../...../.##../..#../..#../..#../.###.',
    'j': '...#./...../..##./...#./...#./...#./...#./#..#./.##..',
    'k': '#..../#..../#..#./#.#../##.../#.#../#..#.',
    'l': '.##../..#../..#../..#../..#../..#../.###.',
    'm': '...../...../##.#./#.#.#/#.#.#/#.#.#/#.#.#',
    'n': '...../...../#.##./##..#/#...#/#...#/#...#',
    'o': '...../...../.###./#...#/#...#/#...#/.###.',
    'p': '...../...../####./#...#/#...#/#...#/####./#..../#....',
    'q': '...../...../.####/#...#/#...#/#...#/.####/....#/....#',
    'r': '...../...../#.##./##..#/#..../#..../#....',
    's': '...../...../.####/#..../.###./....#/####.',
    't': '.#.../.#.../###../.#.../.#.../.#..#/..##.',
    'u': '...../...../#...#/#...#/#...#/#..##/.##.#',
    'v': '...../...../#...#/#...#/#...#/.#.#./..#..',
    'w': '...../...../#...#/#...#/#.#.#/#.#.#/.#.#.',
    'x': '...../...../#...#/.#.#./..#../.#.#./#...#',
    'y': '...../...../#...#/#...#/#...#/#...#/.####/....#/.###.',
    'z': '...../...../#####/...#./..#../.#.../#####',
    '{': '...##/..#../..#../.#.../..#../..#../...##',
    '|': '..#../..#../..#../..#../..#../..#../..#..',
    '}': '##.../..#../..#../...#./..#../..#../##...',
    '~': '...../...../.#..#/#.#.#/#..#./...../.....',
}


def _font_table():
    """uint8 [95, FONT_H]: row bytes of the glyphs of ASCII 32..126, bit x = column x."""
    tab = np.zeros((95, FONT_H), dtype=np.uint8)
    for code in range(32, 127):
        rows = _GLYPHS[chr(code)].split('/')
        if len(rows) not in (7, 9) or any(len(r) != 5 or set(r) - set('.#') for r in rows):
            raise ValueError(f'font: glyph {chr(code)!r} is not 5 x 7 (or 5 x 9) dots')
        for y, r in enumerate(rows):
            tab[code - 32, 1 + y] = sum(1 << x for x, ch in enumerate(r) if ch == '#')
    return tab


FONT = _font_table()


def _jet():
    """uint8 [256,3] RGB: with v = i / 255, r = clamp(1.5 - |4 v - 3|, 0, 1), g with 2 and b with 1 in place of 3, each channel
    floor(255 c + 0.5), in float64.  A restatement of the Jet map's definition, not checked against OpenCV's table."""
    v = np.arange(256, dtype=np.float64) / 255
    rgb = np.stack([np.clip(1.5 - np.abs(4 * v - k), 0, 1) for k in (3, 2, 1)], axis=1)
    return np.floor(255 * rgb + 0.5).astype(np.uint8)


JET = _jet()


def montage_size(Hp, Wp):
    """(Hm, Wm) of the montage of Hp x Wp tiles."""
    return BAND + Hp + 2 * PAD, 5 * (Wp + PAD) + PAD


def tile_x(k, Wp):
    """Left edge of tile k."""
    return PAD + k * (Wp + PAD)


def glyph_index(ch):
    """Index into FONT of a character; anything outside printable ASCII renders as '?'."""
    return ord(ch) - 32 if 32 <= ord(ch) <= 126 else ord('?') - 32


def layout_labels(texts, Wp):
    """Glyph records [(x, y, glyph)] of one montage's labels.  `texts`: 5 tiles x 2 lines of strings; the part of a string after
    a tab is right-aligned to its tile's right edge (the `L2=...` values), the part before it is left-aligned at the tile's left
    edge.  Line 1 is at y = 0, line 2 at y = FONT_H.  Text is truncated at the tile's right edge, and a left-aligned part one cell
    before the right-aligned part of the same line.  Host code only."""
    if len(texts) != 5 or any(len(t) != 2 for t in texts):
        raise ValueError('layout_labels: expected 5 tiles x 2 lines of strings')
    recs = []
    for k, lines in enumerate(texts):
        x0 = tile_x(k, Wp)
        x1 = x0 + Wp
        fit = Wp // FONT_W                       # whole cells in the tile
        for ln, s in enumerate(lines):
            left, _, right = str(s).partition('\t')
            y = ln * FONT_H
            limit = x1
            if right:
                right = right[:fit]
                xr = x1 - len(right) * FONT_W
                recs += [(xr + i * FONT_W, y, glyph_index(c)) for i, c in enumerate(right)]
                limit = xr - FONT_W
            left = left[:max(0, (limit - x0) // FONT_W)]
            recs += [(x0 + i * FONT_W, y, glyph_index(c)) for i, c in enumerate(left)]
    return recs


def attack_texts(t, scene, infer=None, real=None, l2=(None, None, None)):
    """The reference's label strings of one montage as a 5 x 2 table for `layout_labels`: scene / infer / real = (label, top-1
    probability) or None, l2 = the (prj, infer, real) L2 values or None."""
    def cls(v):
        return '' if v is None else f'{v[0]} ({v[1]:.2f})'

    def dist(v):
        return '' if v is None else f'\tL2={v:.2f}'
    return [(LINE1[0].format(t=t), cls(scene)), (LINE1[1], dist(l2[0])), (LINE1[2], cls(infer) + dist(l2[1])),
            (LINE1[3], cls(real) + dist(l2[2])), (LINE1[4], '')]


_DEVICE_FONT = {}


def _font_on(dev):
    key = (dev.type, dev.index)
    if key not in _DEVICE_FONT:
        _DEVICE_FONT[key] = torch.from_numpy(FONT.copy()).to(dev)
    return _DEVICE_FONT[key]


def _images(name, t, n=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f'spaa_amd.montage builds montages on the GPU only (no CPU fallback): {name} is '
                           f'{"on " + str(t.device) if isinstance(t, torch.Tensor) else type(t).__name__}')
    if t.ndim == 3:
        t = t[None]
    if t.ndim != 4 or t.shape[1] != 3 or (n is not None and t.shape[0] != n):
        raise ValueError(f'{name}: expected [{"N" if n is None else n},3,H,W], got {tuple(t.shape)}')
    return t.detach().to(torch.float32).contiguous()


def attack_montages(cam_scene, prj_adv, cam_infer, cam_real, cp_sz, texts, *, colormap=JET, timings=None):
    """uint8 [N,3,Hm,Wm] montages on the device of prj_adv (Hm = 26 + Hp + 10, Wm = 5 (Wp + 5) + 5, background 255): tiles
    rz(cam_scene), prj_adv[n], rz(cam_infer[n]), rz(cam_real[n]) and the colour-mapped normalised |rz(cam_real[n]) - rz(cam_scene)|,
    rz = centre crop to cp_sz = (h, w) and area resize to prj_adv's own (Hp, Wp); then the labels.
    cam_scene [3,Hs,Ws] (or [1,3,Hs,Ws]), prj_adv [N,3,Hp,Wp], cam_infer [N,3,Hi,Wi], cam_real [N,3,Hr,Wr]: float images in
    [0,1] on one GPU.  `texts`: N tables of 5 x 2 strings (`layout_labels`, `attack_texts`).  `colormap`: uint8 [256,3] RGB.
    Two entry points, four kernels, whatever N.  `timings`: a list that receives (entry point, start event, end event).
    A CPU tensor or a missing library raises."""
    prj = _images('prj_adv', prj_adv)
    n, _, hp, wp = prj.shape
    scene, infer, real = _images('cam_scene', cam_scene, 1), _images('cam_infer', cam_infer, n), _images('cam_real', cam_real, n)
    dev = prj.device
    if any(t.device != dev for t in (scene, infer, real)):
        raise ValueError('attack_montages: all images must be on one device')
    if len(texts) != n:
        raise ValueError(f'attack_montages: {n} montages but {len(texts)} text tables')
    if n > 65535 or wp > 6000:
        raise ValueError(f'attack_montages: at most 65535 montages of tiles at most 6000 wide per call, got {n} of width {wp}')
    ch, cw = (int(v) for v in cp_sz)
    geo = []
    for name, t in (('cam_scene', scene), ('cam_infer', infer), ('cam_real', real)):
        h, w = t.shape[-2:]
        y0, x0 = center_crop_origin(h, w, (ch, cw))
        if ch < 1 or cw < 1 or y0 < 0 or x0 < 0 or y0 + ch > h or x0 + cw > w or max(h, w) > 32768:
            raise ValueError(f'attack_montages: the {ch}x{cw} crop does not fit {name} ({h}x{w})')
        geo.append((h, w, y0, x0))
    lut = np.ascontiguousarray(colormap.cpu().numpy() if isinstance(colormap, torch.Tensor) else colormap)
    if lut.shape != (256, 3) or lut.dtype != np.uint8:
        raise ValueError(f'colormap must be uint8 [256,3], got {lut.dtype} {lut.shape}')
    recs = np.array([(i, *r) for i, tab in enumerate(texts) for r in layout_labels(tab, wp)], dtype=np.int32).reshape(-1, 4)
    hm, wm = montage_size(hp, wp)
    p = _lib.ptr

    def launch(name, *args):
        if timings is None:
            return _lib.call(name, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.call(name, *args)
        e1.record()
        timings.append((name, e0, e1))

    with _lib.on_device(dev):
        lut_d = torch.from_numpy(lut.copy()).to(dev)
        recs_d = torch.from_numpy(recs).to(dev) if len(recs) else None
        font_d = _font_on(dev)
        minmax = torch.empty(n, 2, device=dev)
        out = torch.empty(n, 3, hm, wm, dtype=torch.uint8, device=dev)
        launch('spaa_montage_diff_range', p(scene), *geo[0], p(real), *geo[2], n, ch, cw, hp, wp, p(minmax))
        launch('spaa_montage_compose', p(scene), *geo[0], p(prj), p(infer), *geo[1], p(real), *geo[2], n, ch, cw, hp, wp, p(minmax),
               p(lut_d), p(recs_d), len(recs), p(font_d), FONT_W, FONT_H, p(out))
    return out


def diff_range(cam_scene, cam_real, cp_sz, tile_sz):
    """float32 [N,2] on the device: per image of cam_real, min and max of |rz(cam_real[n]) - rz(cam_scene)| over the three channels
    of the tile_sz = (Hp, Wp) tile (spaa_montage_diff_range on its own; attack_montages runs it itself)."""
    real = _images('cam_real', cam_real)
    scene = _images('cam_scene', cam_scene, 1)
    n, (ch, cw), (hp, wp) = real.shape[0], (int(v) for v in cp_sz), (int(v) for v in tile_sz)
    geo = []
    for name, t in (('cam_scene', scene), ('cam_real', real)):
        h, w = t.shape[-2:]
        y0, x0 = center_crop_origin(h, w, (ch, cw))
        if ch < 1 or cw < 1 or y0 < 0 or x0 < 0 or y0 + ch > h or x0 + cw > w or max(h, w) > 32768:
            raise ValueError(f'diff_range: the {ch}x{cw} crop does not fit {name} ({h}x{w})')
        geo.append((h, w, y0, x0))
    with _lib.on_device(real.device):
        minmax = torch.empty(n, 2, device=real.device)
        _lib.call('spaa_montage_diff_range', _lib.ptr(scene), *geo[0], _lib.ptr(real), *geo[1], n, ch, cw, hp, wp, _lib.ptr(minmax))
    return minmax
