"""Plain-torch float64 restatement of the plain conv GEMMs -- dx_conv1d / dx_conv1d_wfrag, dx_conv1d_relu_bits and dx_conv1d_wide of
include/daft_exprt_hip.h -- the cases of tests/test_gpu_conv_plain.py with their operand draws, and the low-precision restatement that
sizes the tolerances of its rounded tests.  Test infrastructure: nothing in the package imports this.  Everything runs on the CPU.

THE CONTRACT, as read from the three kernels (csrc/conv_gemm_kernel.h without a LayerNorm epilogue, csrc/conv_wreg.hip,
csrc/conv_wide.hip); x (B, N, Cin), w (Cout, Cin, taps) = what pack_conv_weight packs, rows outside [0, N) are zero padding:

    v = bias[co] + sum_{tap, ci} x[b, n + tap - taps / 2, ci] * w[co, ci, tap]          (fp32 accumulation of exact products)
    v = max(v, 0)                                   with ReLU
    v = v where gate[b, n, co] > 0, else 0          the gate lies exactly like the output; relu_bits: the bit of the element instead
    v = 0 on rows n >= mask_lengths[b]
    v = v + out[b, n, co]                           under ACCUMULATE (the old value, in the output's type)
    out = round(v)                                  fp32, or bf16 round-to-nearest-even (`store8<bf16_t>` is a plain cast)

ROWS under skip_lengths (len = skip_lengths[b], fe = tests.util.fill_end(len, N) = dx_fill_end; without skip_lengths every row is
computed and nothing below applies):
    kernel              computed rows                                   zero rows                      unspecified
    tiled (BM rows)     tiles starting below len + 2: the full conv     later tiles starting below fe  at or past fe
    tiled, transposed   the same                                        every later tile, up to N      none: (B, Cout, N) is complete
    tiled, ACCUMULATE   the same                                        none: a dead tile is untouched at or past fe
    register weights    as tiled, BM = 128                              as tiled                       at or past fe
    wide                rows below len + 2 (the plan's halo)            [len + 2, fe)                  at or past fe
A live tile computes ALL its rows from the inputs it finds, so the inputs hold values on [0, len + 2), the zeros their producers leave
on [len + 2, fe) and NaN at and past fe (`dress`): no kernel reads there.  With ACCUMULATE the oracle is `computed v, 0 elsewhere` +
old on every row, which says "untouched" for the dead tiles.  relu_bits: word (b, co / 32, n) holds the bit of channel c = co % 32 at
`bit_of(c)` (the register order of conv_wreg_kernel after its lane swaps), 0 on rows >= mask_lengths; dead tiles leave their words
unwritten.

INTEGER DRAWS make the comparison exact: x, w, bias, gate and the old output are small integers from formulas that are symmetric in
no pair of their indices; every partial sum stays below 2^24 so fp32 accumulation is exact in any order (tests/test_conv_plain_host.py
proves it).  Draw 'small' (x, w in {-1, 0, 1}, sparse) keeps every output an integer of magnitude <= 256 -- exact in bf16, so the
rounding cannot hide an off-by-one; draw 'big' (|x| <= 7, |w| <= 6) sends bf16 outputs through the rounding.  GAUSSIAN DRAWS feed the
rounded tests; `restate` is the fp32 computation that rounds where the kernels round: x to bf16 when it is staged in front of bf16
weights, the contraction as an MFMA chain (conv_ln_oracle.conv_chain: K-step 16, or the fp32 products of K-step 2 with fp32 weights),
the output store.
"""
import functools
import types

import torch

from tests import conv_ln_oracle as K
from tests.util import fill_end

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
WREG, ROWS64, ROWS128, ROWS256 = range(4)                  # DX_PLAIN_PATH_* of include/daft_exprt_hip.h
WIDE = 4                                                   # dx_conv1d_wide: chosen by ops.conv1d, not by the query
PATH_NAME = {WREG: 'wreg', ROWS64: 'rows64', ROWS128: 'rows128', ROWS256: 'rows256', WIDE: 'wide'}
TILE_ROWS = {WREG: 128, ROWS64: 64, ROWS128: 128, ROWS256: 256}
# the operand ladders of conv_plain_launch: (x, w, y, gate)
LADDERS = {'f32': (F32, F32, F32, F32), 'mix': (F32, BF16, F32, F32), 'mixg': (F32, BF16, F32, BF16), 'mixb': (F32, BF16, BF16, BF16),
           'bf32': (BF16, BF16, F32, F32), 'bf16': (BF16, BF16, BF16, BF16)}
CAP = K.CAP            # tests/test_conv_plain_host.py holds the Gaussian cases to it ('fp32' / 'mixed' / 'bf16') and writes down what it measured
PAD_LEFT = 8           # a sliced operand starts 8 elements into its NaN container (16-byte alignment of the vector accesses)


def _case(name, path, B, N, lens, Cin, Cout, taps, ladder, **o):
    ''' options: relu, gate, mask, skip, trans, accum, nobias, xpad / ypad (extra elements per row of the container the operand is a slice
        of; ypad 12 makes ldy % 8 != 0), frag (fragment-order copy), bits ('out' | 'in'), tiles (explicit plan size) '''
    known = {'relu', 'gate', 'mask', 'skip', 'trans', 'accum', 'nobias', 'xpad', 'ypad', 'frag', 'bits', 'tiles'}
    assert set(o) <= known, o
    if ladder == 'mixg':
        o['gate'] = True                  # (without a gate the ladder is 'mix')
    return types.SimpleNamespace(name=name, path=path, B=B, N=N, lens_spec=lens, Cin=Cin, Cout=Cout, taps=taps, ladder=ladder,
                                 **{k: o.get(k, 0 if k in ('xpad', 'ypad') else (None if k in ('bits', 'tiles') else False)) for k in known})


# option rows that rotate over the tiled cases: each appears on each tile height and, where it can, on both epilogues
OPTS = [dict(), dict(relu=True), dict(gate=True), dict(relu=True, gate=True, mask=True), dict(mask=True, skip=True),
        dict(trans=True), dict(trans=True, skip=True, relu=True), dict(accum=True), dict(accum=True, skip=True, mask=True),
        dict(nobias=True, relu=True), dict(xpad=16, ypad=16), dict(ypad=12, gate=True, skip=True), dict(accum=True, xpad=8, ypad=16, gate=True),
        dict(trans=True, gate=True, ypad=12, mask=True), dict(accum=True, ypad=12, nobias=True)]


def _drawn_lens(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, N + 1, (B,), generator=g)
    lens[0], lens[1], lens[2], lens[-1] = N, 0, 1, N
    return lens.tolist()


def _tiled_cases():
    out, k = [], 0
    lad = list(LADDERS)
    couts = [128, 80, 8, 1, 7, 33]
    # P1: 64-row tiles.  Cin 8 / 40: one partial K chunk; 128: whole chunks; 160: whole chunks and no multiple of 64.  Cout 128 / 80 / 8: the
    # vector epilogue with a full and a partial channel tile; 1 / 7 / 33: the scalar epilogue
    for li, l in enumerate(lad):
        for ti, taps in enumerate((1, 3)):
            for ci, cin in enumerate((8, 40, 128, 160)):
                cout = couts[(ci + 2 * ti + li) % 6]
                out.append(_case(f'P1-{l}-k{taps}-C{cin}-O{cout}', ROWS64, 3, 70, [70, 33, 1], cin, cout, taps, l, **OPTS[k % len(OPTS)]))
                k += 1
    # P2: 128-row tiles (two or three channel tiles; Cout 136: the second one holds 8 channels)
    combos = [(40, 136), (136, 264), (136, 136), (40, 264)]
    for li, l in enumerate(lad):
        for ti, taps in enumerate((1, 3)):
            for j in range(2):
                cin, cout = combos[(2 * ti + j + li) % 4]
                out.append(_case(f'P2-{l}-k{taps}-C{cin}-O{cout}', ROWS128, 2, 131, [131, 64], cin, cout, taps, l, **OPTS[k % len(OPTS)]))
                k += 1
    out.append(_case('P2-f32-k3-C512-O136', ROWS128, 2, 131, [131, 64], 512, 136, 3, 'f32', relu=True))     # fp32 weights at Cin 512 stay
    # the scalar epilogue on 128-row tiles: Cout 135 (second channel tile: 7 channels)
    out.append(_case('P2-bf16-k3-C40-O135', ROWS128, 2, 131, [131, 64], 40, 135, 3, 'bf16', gate=True, mask=True))
    out.append(_case('P2-f32-k1-C40-O135', ROWS128, 2, 131, [131, 64], 40, 135, 1, 'f32', accum=True))
    # P3: 128-row tiles of the narrow form (one channel tile, more than 64000 rows)
    for (cin, cout), l, o in zip([(8, 8), (40, 128), (8, 128), (40, 8)], ('f32', 'bf16', 'mixb', 'bf32'),
                                 (dict(skip=True, relu=True), dict(gate=True, mask=True), dict(accum=True, skip=True), dict(ypad=12))):
        out.append(_case(f'P3-{l}-C{cin}-O{cout}', ROWS128, 167, 385, 'drawn', cin, cout, 3, l, **o))
    # P4': 256-row tiles by the workgroup count
    out.append(_case('P4n-bf16-O256', ROWS256, 512, 3, 'drawn', 512, 256, 3, 'bf16', relu=True, skip=True))
    out.append(_case('P4n-bf32-O256', ROWS256, 512, 3, 'drawn', 512, 256, 3, 'bf32', gate=True, mask=True))
    # P5: a tile that starts past len + 2 below AND past the fill end (lens 255 / 1 / 0 at N 600: fill end 513 / 257 / 257)
    l5 = [600, 255, 1, 0]
    for path, cout, l, o in ((ROWS64, 8, 'f32', dict()), (ROWS64, 7, 'bf16', dict()), (ROWS64, 8, 'bf16', dict(accum=True)),
                             (ROWS64, 7, 'f32', dict(accum=True, mask=True)), (ROWS64, 8, 'mixb', dict(trans=True)),
                             (ROWS128, 136, 'bf16', dict(relu=True)), (ROWS128, 135, 'mix', dict(gate=True)),
                             (ROWS128, 136, 'bf32', dict(accum=True)), (ROWS128, 136, 'f32', dict(trans=True, mask=True))):
        out.append(_case(f'P5-{PATH_NAME[path]}-{l}-O{cout}' + ''.join('-' + a for a in o), path, 4, 600, l5, 8, cout, 3, l, skip=True, **o))
    return out


def _tall_cases():
    ''' P4: 256-row tiles forced with DX_CONV_WIDE_MI = 4 (a fresh child process runs them) '''
    out = []
    rows = [('bf16', 256, dict(relu=True, mask=True)), ('bf32', 264, dict(gate=True, skip=True)), ('mix', 256, dict(accum=True, skip=True)),
            ('mixb', 264, dict(trans=True, skip=True)), ('mixg', 256, dict(xpad=16, ypad=16)), ('bf16', 263, dict(accum=True, gate=True)),
            ('bf16', 264, dict(nobias=True, ypad=12, skip=True, mask=True)), ('bf32', 256, dict(trans=True, relu=True))]
    for l, cout, o in rows:
        out.append(_case(f'P4-{l}-O{cout}' + ''.join('-' + a for a in o), ROWS256, 3, 300, [300, 257, 5], 512, cout, 3, l, **o))
    out.append(_case('P5-rows256-bf16-O264', ROWS256, 4, 600, [600, 255, 1, 0], 512, 264, 3, 'bf16', skip=True))
    out.append(_case('P5-rows256-bf32-O256-accum', ROWS256, 4, 600, [600, 255, 1, 0], 512, 256, 3, 'bf32', skip=True, accum=True))
    return out


def _wreg_cases():
    out, k = [], 0
    shapes = [('R1', 3, 300, [300, 130, 5]), ('R2', 8, 100, [100, 99, 64, 33, 100, 1, 17, 80]), ('R3', 513, 3, 'drawn'),
              ('R4', 4, 600, [600, 0, 1, 255])]
    forms = [dict(), dict(relu=True), dict(gate=True), dict(relu=True, gate=True)]
    extra = [dict(skip=True), dict(mask=True), dict(skip=True, mask=True), dict(nobias=True, skip=True)]
    for si, (name, B, N, lens) in enumerate(shapes):
        for comb, (l, taps) in enumerate((l, t) for l in ('bf16', 'bf32') for t in (1, 3)):
            # over the four shapes every (output type, tap count) meets each of the four ReLU / gate forms: all 16 instantiations
            o = dict(forms[(si + comb) % 4], **extra[(si + 2 * comb) % 4])
            if name == 'R4':
                o['skip'] = True
            out.append(_case(f'{name}-{l}-k{taps}' + ''.join('-' + a for a in o), WREG, B, N, lens, 128, (256, 512)[k % 2], taps, l,
                             frag=(taps == 3 and si % 2 == 0), xpad=(8 if k % 5 == 0 else 0), ypad=(16 if k % 5 == 0 else 0), **o))
            k += 1
        for bits in ('out', 'in'):           # dx_conv1d_relu_bits: ReLU forward that leaves the bits, data gradient gated by the bits
            out.append(_case(f'{name}-bits-{bits}', WREG, B, N, lens, 128, (512, 256)[k % 2], 3, 'bf16', bits=bits, relu=bits == 'out',
                             nobias=bits == 'in', skip=True, mask=k % 3 != 0, frag=k % 2 == 0))
            k += 1
    return out


def _wide_cases():
    out, k = [], 0
    shapes = [('W1', 4, 128, [128, 96, 33, 1], None), ('W2', 3, 300, [300, 252, 0], None), ('W3', 70, 40, 'drawn', None),
              ('W4', 4, 128, [128, 96, 33, 1], 4)]
    for name, B, N, lens, tiles in shapes:
        for cin in (256, 384):
            for cout in (256, 512):
                out.append(_case(f'{name}-C{cin}-O{cout}', WIDE, B, N, lens, cin, cout, 3, 'bf16', skip=True, relu=k % 2 == 0,
                                 nobias=(k // 2) % 2 == 1 or k % 5 == 0, tiles=tiles, xpad=(16 if k % 3 == 0 else 0)))
                k += 1
    return out


TILED, TALL, WREG_CASES, WIDE_CASES = _tiled_cases(), _tall_cases(), _wreg_cases(), _wide_cases()
ALL = {c.name: c for c in TILED + TALL + WREG_CASES + WIDE_CASES}
assert len(ALL) == len(TILED) + len(TALL) + len(WREG_CASES) + len(WIDE_CASES), 'case names must be unique'
# the rounded tests: one case per kernel path, operand ladder and tap count (Gaussian operands)
ROUNDED = ([_case(f'G-rows64-{l}-k{t}', ROWS64, 3, 70, [70, 33, 1], 160, 80, t, l, relu=True, gate=(l == 'mixg'), skip=True) for l in LADDERS for t in (1, 3)]
           + [_case(f'G-rows128-{l}-k{t}', ROWS128, 2, 131, [131, 64], 136, 136, t, l, mask=True) for l in LADDERS for t in (1, 3)]
           + [_case(f'G-wreg-{l}-k{t}', WREG, 3, 300, [300, 130, 5], 128, 256, t, l, relu=(t == 3), skip=True, frag=(t == 3)) for l in ('bf16', 'bf32') for t in (1, 3)]
           + [_case(f'G-wide-C{cin}', WIDE, 3, 300, [300, 252, 0], cin, 256, 3, 'bf16', skip=True, relu=(cin == 384)) for cin in (256, 384)])
ROUNDED_TALL = [_case(f'G-rows256-{l}', ROWS256, 3, 300, [300, 257, 5], 512, 264, 3, l, skip=True) for l in ('mix', 'mixb', 'bf32', 'bf16')]
ALL_ROUNDED = {c.name: c for c in ROUNDED + ROUNDED_TALL}


# ----------------------------------------------------------------------------- draws
def lengths_of(c):
    if c.lens_spec == 'drawn':
        return _drawn_lens(c.B, c.N, 100 + c.B + c.N)
    return list(c.lens_spec)


def _grid(*sizes):
    return torch.meshgrid(*[torch.arange(s, dtype=torch.int64) for s in sizes], indexing='ij')


def hx(b, n, ci):
    ''' the index hash of x: symmetric in no pair of (b, n, ci) '''
    return (3 * b + 5 * n + 11 * ci + 7 * b * n + 13 * n * ci + 17 * b * ci + n * n) % 251


def hw(co, ci, tap):
    return (7 * co + 3 * ci + 29 * tap + 5 * co * ci + 19 * ci * tap + 23 * co * tap + ci * ci + 2 * co * co) % 241


def hg(b, n, co):
    return (5 * b + 3 * n + 7 * co + 11 * b * n + 2 * n * co + 13 * b * co + co * co) % 239


def ho(b, n, co):
    return (11 * b + 7 * n + 3 * co + 5 * b * n + 3 * n * co + 2 * b * co + n * n + b) % 233


def _small(h):
    ''' {-1, 0, 1}, two sevenths non-zero '''
    r = h % 7
    return (r == 1).long() - (r == 4).long()


def draw_x(c, draw, B, N, Cin, perm=(0, 1, 2)):
    ''' perm: the index roles handed to the formula (the host test swaps two of them) '''
    idx = _grid(B, N, Cin)
    h = hx(*[idx[p] for p in perm])
    return (_small(h) if draw == 'small' else h % 15 - 7).double()


def draw_w(c, draw, Cout, Cin, taps, perm=(0, 1, 2)):
    idx = _grid(Cout, Cin, taps)
    h = hw(*[idx[p] for p in perm])
    return (_small(h) if draw == 'small' else h % 13 - 6).double()


def dress(t, lens, N, nan=True, zero=True):
    ''' (B, N, ...) float tensor: rows of [len + 2, fe) zero, rows at and past fe NaN '''
    L = torch.tensor(lens)
    n = torch.arange(N)[None, :]
    if zero:
        t[(n >= L[:, None] + 2).expand(t.shape[:2])] = 0.
    if nan:
        t[(n >= fill_end(L, N)[:, None]).expand(t.shape[:2])] = float('nan')
    return t


def make_case(c, draw, xperm=(0, 1, 2), wperm=(0, 1, 2), gperm=(0, 1, 2), operm=(0, 1, 2)):
    ''' the operands of case c on the CPU in their storage types: draw 'small' | 'big' (integers) | 'gauss' '''
    x_dt, w_dt, y_dt, g_dt = LADDERS[c.ladder]
    B, N, Cin, Cout, taps = c.B, c.N, c.Cin, c.Cout, c.taps
    lens = lengths_of(c)
    m = types.SimpleNamespace(c=c, draw=draw, lens=lens, L=torch.tensor(lens, dtype=torch.int64), x_dt=x_dt, w_dt=w_dt, y_dt=y_dt, g_dt=g_dt)
    m.fe = fill_end(m.L, N).tolist() if c.skip else [N] * B
    m.mask_lens = [min(l + 1, N) for l in lens] if c.mask else None
    if draw == 'gauss':
        g = torch.Generator().manual_seed(7000 + 8 * Cin + Cout + taps + 31 * B)
        x = torch.randn(B, N, Cin, generator=g).double()
        w = (torch.randn(Cout, Cin, taps, generator=g) / (Cin * taps) ** 0.5).double()
        bias = torch.randn(Cout, generator=g).double()
        gate = torch.randn(B, N, Cout, generator=g).double()
        old = torch.randn(B, N, Cout, generator=g).double()
    else:
        x, w = draw_x(c, draw, B, N, Cin, xperm), draw_w(c, draw, Cout, Cin, taps, wperm)
        co = torch.arange(Cout)
        bias = ((co * 3 + co * co) % 7 - 3).double()
        idx = _grid(B, N, Cout)
        gate = (hg(*[idx[p] for p in gperm]) % 5 - 2).double()
        old = (ho(*[idx[p] for p in operm]) % 9 - 4).double()
    if c.skip:
        x, gate = dress(x, lens, N), dress(gate, lens, N)
        # the old output keeps its integers on the dead rows below the fill end: a dead tile must leave them as they are, and zeros there
        # could not tell "untouched" from "zero-filled".  (The transposed form is complete: its old value is finite everywhere.)
        old = dress(old, lens, N, nan=not c.trans, zero=False)
    m.x = x.to(x_dt)
    m.w = w.to(w_dt).float()              # rounded to its storage type here: the packed operand holds exactly these numbers
    m.bias = None if c.nobias else bias.float()
    m.gate = gate.to(g_dt) if (c.gate or c.bits == 'in') else None
    m.old = old.to(y_dt) if c.accum else None
    return m


# ----------------------------------------------------------------------------- the contract
def computed_rows(m):
    ''' (B, N) bool: the rows the kernel computes; the others are zero (untouched under ACCUMULATE) below the fill end '''
    c = m.c
    n = torch.arange(c.N)[None, :]
    if not c.skip:
        return torch.ones(c.B, c.N, dtype=torch.bool)
    if c.path == WIDE:
        return n < (m.L[:, None] + 2)
    return n < torch.tensor([K.live_end(l, c.N, TILE_ROWS[c.path]) for l in m.lens])[:, None]


def contract_rows(m):
    ''' (B, N) bool: the rows a test may look at (everything for the transposed form) '''
    c = m.c
    if c.trans or not c.skip:
        return torch.ones(c.B, c.N, dtype=torch.bool)
    return torch.arange(c.N)[None, :] < torch.tensor(m.fe)[:, None]


def _clean(t, T):
    return torch.nan_to_num(t.to(T), nan=0.)


def _epilogue(m, v, T):
    c = m.c
    if m.bias is not None:
        v = v + m.bias.to(T)
    if c.relu:
        v = torch.relu(v)
    if m.gate is not None:
        v = torch.where(_clean(m.gate, T) > 0, v, torch.zeros_like(v))
    if m.mask_lens is not None:
        v = v.masked_fill((torch.arange(c.N)[None, :] >= torch.tensor(m.mask_lens)[:, None])[:, :, None], 0.)
    v = v.masked_fill(~computed_rows(m)[:, :, None], 0.)
    if m.old is not None:
        v = v + _clean(m.old, T)
    return v


def reference(m, x=None, w=None):
    ''' THE reference: float64, unrounded, (B, N, Cout) '''
    return _epilogue(m, K.conv(_clean(m.x, F64) if x is None else x, m.w if w is None else w), F64)


def reference_stored(m):
    ''' the reference rounded to the output's type (integer draws: what the kernel must store, bit for bit) '''
    return reference(m).to(F32).to(m.y_dt)


def restate(m):
    ''' fp32 with the kernels' roundings, unrounded output and the output as stored '''
    xs = _clean(m.x, F32)
    if m.w_dt == BF16:
        v = K.conv_chain(xs.to(BF16).float(), m.w, 16)
    else:
        v = K.conv_chain(xs, m.w, 2, fp32_products=True)
    v = _epilogue(m, v, F32)
    return v.to(m.y_dt).double()


def kind_of(m):
    ''' which cap of conv_ln_oracle.CAP limits the Gaussian case '''
    if m.y_dt == BF16:
        return 'bf16'
    return 'mixed' if (m.x_dt, m.w_dt) == (F32, BF16) else 'fp32'


@functools.lru_cache(maxsize=None)
def integer_case(name, draw):
    ''' (operands, reference as stored) of an integer case, computed once '''
    m = make_case(ALL[name], draw)
    return m, reference_stored(m)


@functools.lru_cache(maxsize=None)
def gauss_case(name):
    m = make_case(ALL_ROUNDED[name], 'gauss')
    return m, reference(m), restate(m)


# ----------------------------------------------------------------------------- relu_bits
def bit_of(ch):
    ''' bit of channel ch (0..31 inside its 32-channel block) in a relu_bits word: conv_wreg_kernel's register order -- after the lane swaps
        lane group g = (ch % 16) // 8 holds channel pairs, register k = 4 * (ch // 16) + (ch % 8) // 2, low / high half = ch % 2; group 0
        sits in bits 0-7 / 16-23 of the word, group 1 in 8-15 / 24-31 '''
    return 16 * (ch % 2) + 8 * ((ch % 16) // 8) + 4 * (ch // 16) + (ch % 8) // 2


def pack_bits(pos):
    ''' (B, N, Cout) bool -> int32 (B, Cout / 32, N) '''
    B, N, C = pos.shape
    sh = torch.tensor([bit_of(ch) for ch in range(32)], dtype=torch.int64)
    words = (pos.view(B, N, C // 32, 32).long() << sh).sum(dim=3)                   # (B, N, C / 32), below 2^32
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)
    return words.permute(0, 2, 1).contiguous().to(torch.int32)


# ----------------------------------------------------------------------------- what a case reaches (the kernels' arithmetic, restated)
def cdiv(a, b):
    return -(-a // b)


def tiled_geometry(c, lens, BM):
    ''' position tiles, channel tiles, and per utterance the number of live / zero-filled / unwritten tiles of the tiled kernel '''
    pt = cdiv(c.N, BM)
    live = [min(pt, cdiv(min(c.N, l + 2), BM)) if c.skip else pt for l in lens]
    fe = fill_end(torch.tensor(lens), c.N).tolist()
    zero = [sum(1 for t in range(lv, pt) if t * BM < f or c.trans) for lv, f in zip(live, fe)]
    return types.SimpleNamespace(ptiles=pt, ztiles=cdiv(c.Cout, 128), live=live, zero=zero, unwritten=[pt - a - z for a, z in zip(live, zero)],
                                 partial_chunk=c.Cin % 32 != 0, chunks=cdiv(c.Cin, 32), vec_out=(not c.trans and c.Cout % 8 == 0 and ldy_of(c) % 8 == 0))


def ldy_of(c):
    return (c.N if c.trans else c.Cout) + c.ypad


def ldx_of(c):
    return c.Cin + c.xpad


def wreg_geometry(c, lens):
    ''' try_weight_stationary / conv_wreg_kernel: groups, order, scan, and the share [i0, i1) of the live tiles each group walks '''
    pt = cdiv(c.N, 128)
    zt = c.Cout // 256
    ngrp = max(1, min(256 // zt, pt * c.B))
    live = [min(pt, cdiv(min(c.N, l + 2), 128)) if c.skip else pt for l in lens]
    total = sum(live)
    shares = [(total * g // ngrp, total * (g + 1) // ngrp) for g in range(ngrp)]
    owner = [b for b, lv in enumerate(live) for _ in range(lv)]                       # utterance of live tile i
    crossing = sum(1 for i0, i1 in shares if i1 > i0 and len({owner[i] for i in range(i0, i1)}) > 1)
    fe = fill_end(torch.tensor(lens), c.N).tolist()
    dead_zero = sum(1 for lv, f in zip(live, fe) for t in range(lv, pt) if t * 128 < f) if c.skip else 0
    dead_unwritten = (pt * c.B - total - dead_zero) if c.skip else 0
    return types.SimpleNamespace(ptiles=pt, ztiles=zt, ngrp=ngrp, zmajor=ngrp % 8 == 0, scan=c.B <= 512, total=total, shares=shares,
                                 crossing=crossing, max_share=max(i1 - i0 for i0, i1 in shares), dead_zero=dead_zero,
                                 dead_unwritten=dead_unwritten, idle_groups=sum(1 for i0, i1 in shares if i1 == i0))


def wide_plan_tiles(c):
    worst = c.B * cdiv(c.N, 256)
    return max(int(c.tiles), worst) if c.tiles is not None else cdiv(worst, 64) * 64
