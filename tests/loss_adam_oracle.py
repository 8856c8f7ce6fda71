"""Float64 oracle of the tail of the training step -- csrc/train_ops.hip (dx_loss_fwd_bwd, dx_sumsq, dx_adam_step, dx_step_scalars_set)
and csrc/adam_pack.hip (dx_adam_pack_step) -- in numpy, without autograd and without a GPU.  tests/test_loss_adam_host.py holds it
against float64 autograd / torch.optim.Adam and its restated launch geometry against the library; tests/test_gpu_loss_adam.py holds
the kernels against it.

Conventions
  * The inputs are the kernels' fp32 arrays, taken as exact.  Scalars that reach a kernel as `float` (loss weights, grad_scale, lr,
    betas, eps, weight decay, clipping threshold, the 1e-6 of clip_grad_norm_) are rounded to fp32 first and `1 - beta` is formed
    from the rounded beta: `1 - 0.98f` alone is 16 u away from 0.02, relatively.  bc1 = float32(1 - b1^t) and bc2_sqrt =
    float32(sqrt(1 - b2^t)) are computed in double from the rounded betas, as dx_adam_step and dx_step_scalars_set do.
  * The padding counts (loss.py:54-99 relies on zero padding and masks nothing): sums run over all of L / T and are divided by
    length_b * B, the mel sums by n_mel * out_len_b * B.
  * d_post accumulates (`+=`), every other gradient is written; everything is scaled by grad_scale.

Error bounds (u = 2^-24, the unit roundoff of fp32; division and sqrtf are correctly rounded in this build: no fast-math flag)
  * A loss term other than terms[0], and every sum of squares, adds non-negative numbers: however the additions are ordered, the
    result is within (K + c) u of the exact sum, relatively, where K is the longest chain of fp32 additions a summand passes through
    and c counts the roundings of one summand and of the scaling behind the sum.  K is computed from the launch geometry restated
    below (`loss_chains`, `sumsq_geometry`, `adam_chain`, `adam_pack_chain`): per-thread trips, 6 butterfly steps of the wave, 4 wave
    partials, then the atomics (one chain link per workgroup) or the partials that the last launch sums (trips + 6 + 4 again).
        c = 8 for the loss terms: the difference (1), its square (1; |d| has none), `w * acc` (1), `* inv` (1), and
            inv = 1 / ((float)C * (float)len * (float)B): two products and the division (3; the sequence terms have one product) --
            7 at most, one spare for terms[1], where the sqrtf (1) and `w_post * nrm` (1) follow a sum whose error the root halves;
        c = 1 for the sums of squares (the product).
    The bound is taken as (K + c) u / (1 - (K + c) u), which covers the second-order terms.
  * Gradients and Adam outputs are element-wise and cancel (`b1 m + (1 - b1) g`, `softmax - onehot`), so they are bounded by a count of
    roundings times u times the sum of the ABSOLUTE values of the addends, never relative to the result:
        d_dur / d_energy / d_pitch   6 u |g|   difference, gscale * w, * d, * inv, and the two roundings of inv (* 2 is exact)
        d_mel                        8 u |g|   difference, sign + 2 d, gscale * w, *, * inv, and the three roundings of inv
        d_post                       (K_post + 5) u |g| + u (|old| + |g|)   the norm's sum and root, gscale * w, * post, / nrm; then `+=`
        Adam                         first-order propagation through the kernel's expression, `adam` below:
            G  = |g coef| + |wd p|                                   e_g = 5 u G          (coef: sqrt, +, /; g * coef; wd * p; +)
            Am = |b1 m| + (1 - b1) G                                 e_m = 8 u Am
            Av = b2 v + (1 - b2) G^2                                 e_v = 14 u Av        (gi^2 carries 2 G e_g)
            r = sqrt(v'): e_r = min(e_v / 2r, sqrt(e_v)) + u r;  D = r / bc2_sqrt + eps: e_D = (e_r + u r) / bc2_sqrt + u D
            U = step m' / D: e_U = 3 u |U| + step e_m / D + |U| e_D / (D - e_D);        p' = p - U: e_p = e_U + u (|p| + |U|)
  * expf / logf enter only terms[0] and d_spk.  Their accuracy is not stated in the documentation ROCm installs, so the bound carries
    it as a parameter E (ulps per call, the same for both) and is otherwise derived: with a_s = z_s - max z (one rounding: the
    exponential turns it into a relative error |a_s| u),
        rel(se)   = sum_s e^{a_s} (|a_s| + 2 E) / se + S        (S additions)
        err(ce_b) = u (rel(se) + 2 E |log se| + |mx + log se| + |ce_b|) + S 2^-126
        terms[0]  : w / B (sum_b err(ce_b) + (K_ce + 2) u sum_b |ce_b|)
        d_spk     : gscale w / B u (p_s (|a_s| + 2 E + rel(se) + 1) + 4 (p_s + onehot)) + 2^-126       (2^-126: a result flushed to zero)
    The value of E the GPU test uses is measured; DESIGN.md has the figure and the margin.
"""
import math
from collections import namedtuple

import numpy as np

U32 = 2. ** -24
TINY = 2. ** -126
F = np.float32


def f32(x):
    return float(np.float32(x))


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------- launch geometry, restated
MT_T, MT_CMAX, MT_TPW = 64, 128, 4            # mel_loss_t_kernel: frames per tile, most channels, tiles per workgroup without ws
FLAT_BLOCK = 4096                             # adam_pack_kernel: elements of a flat range per workgroup
PACK_DESC_BYTES, FLAT_DESC_BYTES = 64, 24     # AdamPackDesc, AdamFlatDesc
SUMSQ_GRID_CAP, GRID_CAP = 1024, 2048         # dx_sumsq's grid_for(n / 8 + 1, 1024); grid_for's default cap (dx_adam_step)
BLOCK = 256
REDUCE = 6 + 4                                # dx_block_sum<4>: the wave butterfly, then the four wave partials
C_TERM, C_SQ = 8, 1


def grid_for(total, cap=GRID_CAP):
    return max(1, min(cap, cdiv(total, BLOCK)))


def loss_ws_floats(B, T):
    return 0 if B <= 0 or T <= 0 else 3 * B + 2 * B * cdiv(T, MT_T)


def nonneg_bound(K, c):
    ''' relative error of an fp32 sum of non-negative summands: K additions in the longest chain, c roundings per summand '''
    e = (K + c) * U32
    return e / (1. - e)


FORMS = ('plain', 'tws', 'tnows', 'terms')    # gradient as (B, C, T) | transposed with workspace | transposed without | no gradients


def loss_path(form, n_mel):
    ''' (mel kernel, partials) that dx_loss_fwd_bwd takes: 'flat' = mel_loss_kernel, 'flat_t' = the same with dtrans = 1,
        'tile' = mel_loss_t_kernel; partials = the per-workgroup terms go through the workspace instead of atomics '''
    assert form in FORMS
    if form in ('plain', 'terms'):
        return 'flat', False
    if n_mel > MT_CMAX:
        return 'flat_t', False
    return 'tile', form == 'tws'


def loss_chains(B, L, T, n_mel, n_post, form):
    ''' K of every summed term: {'seq', 'mel', 'post', 'ce'} '''
    kernel, part = loss_path(form, n_mel)
    landing = lambda n_addr: (cdiv(n_addr, BLOCK) + REDUCE) if part else n_addr
    seq = cdiv(L, BLOCK) + REDUCE + landing(B)
    if kernel == 'tile':
        tpw = 1 if part else MT_TPW
        mel = tpw * cdiv(n_mel * MT_T, BLOCK) + REDUCE + landing(B * cdiv(T, MT_T * tpw))
    else:
        chunks = min(64, cdiv(n_mel * T, BLOCK * 8))
        mel = cdiv(n_mel * T, chunks * BLOCK) + REDUCE + chunks * B
    return {'seq': seq, 'mel': mel, 'post': cdiv(max(n_post, 1), BLOCK) + REDUCE, 'ce': cdiv(B, BLOCK) + REDUCE}


def sumsq_geometry(n, offset):
    ''' sumsq_kernel on n floats that start `offset` floats behind a 16-byte boundary: head, quads, tail, grid, stride, the most
        unrolled / remainder trips any thread makes, and K '''
    head = min((4 - offset % 4) % 4, n)
    nq = (n - head) >> 2
    tail = n - head - 4 * nq
    grid = grid_for(n // 8 + 1, SUMSQ_GRID_CAP)
    s = grid * BLOCK
    i = np.arange(s, dtype=np.int64)
    un = np.maximum(0, -(-(nq - 3 * s - i) // (4 * s)))
    rem = np.maximum(0, -(-(nq - i - 4 * s * un) // s))
    # the thread whose next unrolled trip would start exactly one quad short (i + 3 s == nq): the one `<=` for `<` sends past the end
    edge = (nq - 3 * s) % (4 * s) if nq >= 3 * s else s
    geo = dict(head=head, nq=nq, tail=tail, grid=grid, stride=s, unrolled=int(un.max()), remainder=int(rem.max()),
               edge_thread=edge if edge < s else None)
    # a quad is three additions and one onto the accumulator; head and tail one trip each; (a0 + a1) + (a2 + a3); the block; the atomics
    geo['K'] = 4 * int((un + rem).max()) + 1 + 2 + REDUCE + grid
    return geo


def sumsq_positions(n, offset):
    ''' where an impulse goes: in the head, the first quad, the last quad of the unrolled loop, the remainder loop, the tail, the end '''
    g = sumsq_geometry(n, offset)
    s, head, nq = g['stride'], g['head'], g['nq']
    pos = {'last': n - 1}
    if head:
        pos['head'] = head - 1
    if nq:
        pos['first_quad'] = head + 2
    if nq > 3 * s:
        # thread i's k-th unrolled trip reads quads i + 4 s k + {0, s, 2 s, 3 s}: the last quad read there is the largest
        # q = i + 4 s k + 3 s below nq with i < s
        q = nq - 1
        r = (q - 3 * s) % (4 * s)
        if r >= s:
            q -= r - (s - 1)
        pos['last_unrolled'] = head + 4 * q + 1
    if g['remainder']:
        # quad q belongs to thread q % s; it is read by the remainder loop when that thread's unrolled trips end at or below it
        q = np.arange(max(0, nq - s), nq, dtype=np.int64)
        un = np.maximum(0, -(-(nq - 3 * s - q % s) // (4 * s)))
        pos['remainder'] = head + 4 * int(q[q // s >= 4 * un].max()) + 3
    if g['tail']:
        pos['tail'] = head + 4 * nq
    return pos


def adam_chain(n):
    ''' K of dx_adam_step's norm_accum: trips, the block, one atomic per workgroup, and the value already there '''
    grid = grid_for(n)
    return cdiv(n, grid * BLOCK) + REDUCE + grid + 1


def adam_pack_chain(weights, flats):
    ''' K of dx_adam_pack_step's norm_accum; weights: [(Cout, Cin, taps)], flats: [n] '''
    blocks = sum(cdiv(co, 32) * cdiv(ci, 32) for co, ci, _ in weights) + sum(cdiv(n, FLAT_BLOCK) for n in flats)
    trips = max([cdiv(32 * 32 * min(t, 3), BLOCK) for _, _, t in weights] + [cdiv(min(n, FLAT_BLOCK), BLOCK) for n in flats])
    return trips + REDUCE + blocks + 1


# ---------------------------------------------------------------------------------------------------- the loss
# (B, L, T, n_mel, S): what each shape is for is asserted in tests/test_loss_adam_host.py
LOSS_SHAPES = {
    'prod': (7, 33, 301, 80, 10),
    'tile': (3, 5, 64, 80, 4),
    'tile1': (3, 5, 65, 80, 4),
    'one': (2, 1, 1, 1, 1),
    'cmax': (4, 300, 130, 128, 3),
    'wide': (2, 9, 70, 130, 3),
    'batch': (257, 3, 5, 4, 2),
}
N_POST = 300              # more than one trip of the 256 threads
WEIGHTS = (0.37, 1.3, 3.0, 0.7, 1.9, 2.3)     # (w_spk, w_post, w_dur, w_energy, w_pitch, w_mel): none representable but 3.0


def loss_problem(name, seed=0, logit_scale=1., grid=False):
    ''' fp32 inputs of dx_loss_fwd_bwd on LOSS_SHAPES[name]: lengths >= 1 with the first one full, values everywhere (the padding
        included).  grid=True: predictions EQUAL to targets, on a grid of quarters (an impulse of 1/2 is then exact) '''
    B, L, T, C, S = LOSS_SHAPES[name]
    r = np.random.default_rng(1000 + seed)
    draw = (lambda *s: (r.integers(-8, 9, s) / 4.).astype(F)) if grid else (lambda *s: r.standard_normal(s).astype(F))
    p = {'shape': (B, L, T, C, S)}
    for k in ('dur', 'energy', 'pitch'):
        p[k + '_t'] = draw(B, L)
        p[k] = p[k + '_t'].copy() if grid else draw(B, L)
    p['mel_t'] = draw(B, C, T)
    p['mel'] = p['mel_t'].copy() if grid else draw(B, C, T)
    p['in_len'] = r.integers(1, L + 1, B).astype(np.int64)
    p['out_len'] = r.integers(1, T + 1, B).astype(np.int64)
    p['in_len'][0], p['out_len'][0] = L, T
    p['in_len'][-1], p['out_len'][-1] = max(1, L // 2), max(1, T // 2)        # padding wherever there is room for it
    p['logits'] = (logit_scale * r.standard_normal((B, S))).astype(F)
    if logit_scale > 1:      # spread over [-scale, scale], both ends in every row that has two classes
        p['logits'] = r.uniform(-logit_scale, logit_scale, (B, S)).astype(F)
        p['logits'][:, 0] = logit_scale
        p['logits'][:, -1] = -logit_scale if S > 1 else logit_scale
    p['ids'] = r.integers(0, S, B).astype(np.int64)
    p['post'] = r.standard_normal(N_POST).astype(F)
    return p


LossResult = namedtuple('LossResult', 'terms grads term_abs spk')


def loss_terms_and_grads(p, weights=WEIGHTS, grad_scale=1., post=True):
    ''' terms (8,) and {'d_dur', 'd_energy', 'd_pitch', 'd_mel' (B, C, T), 'd_spk', 'd_post'} in float64, closed formulas;
        spk = what the bound of terms[0] / d_spk needs (`spk_bounds`) '''
    w_spk, w_post, w_dur, w_energy, w_pitch, w_mel = [f32(w) for w in weights]
    gs = f32(grad_scale)
    B, L, T, C, S = p['shape']
    terms, grads = np.zeros(8), {}
    z = p['logits'].astype(np.float64)
    mx = z.max(axis=1, keepdims=True)
    a = z - mx
    ea = np.exp(a)
    se = ea.sum(axis=1, keepdims=True)
    onehot = np.zeros_like(z)
    onehot[np.arange(B), p['ids']] = 1.
    ce = (mx + np.log(se))[:, 0] - z[np.arange(B), p['ids']]
    terms[0] = w_spk * ce.sum() / B
    grads['d_spk'] = gs * w_spk * (ea / se - onehot) / B
    pm = p['post'].astype(np.float64) if post else None
    if post:
        nrm = math.sqrt(float((pm * pm).sum()))
        terms[1] = w_post * nrm
        grads['d_post'] = gs * w_post * pm / nrm if nrm > 0 else np.zeros_like(pm)
    for i, (k, w) in enumerate((('dur', w_dur), ('energy', w_energy), ('pitch', w_pitch))):
        d = p[k].astype(np.float64) - p[k + '_t'].astype(np.float64)
        inv = 1. / (p['in_len'].astype(np.float64) * B)
        terms[2 + i] = w * ((d * d).sum(axis=1) * inv).sum()
        grads['d_' + k] = gs * w * 2. * d * inv[:, None]
    d = p['mel'].astype(np.float64) - p['mel_t'].astype(np.float64)
    inv = 1. / (C * p['out_len'].astype(np.float64) * B)
    terms[5] = w_mel * (np.abs(d).sum(axis=(1, 2)) * inv).sum()
    terms[6] = w_mel * ((d * d).sum(axis=(1, 2)) * inv).sum()
    grads['d_mel'] = gs * w_mel * (np.sign(d) + 2. * d) * inv[:, None, None]
    terms[7] = terms[:7].sum()
    spk = dict(a=a, ea=ea, se=se, mx=mx, ce=ce, onehot=onehot, w=w_spk, gs=gs, B=B, S=S)
    return LossResult(terms, grads, np.abs(terms[:7]).sum(), spk)


def spk_bounds(spk, K_ce, E):
    ''' absolute bounds of terms[0] and of d_spk (module docstring) with expf / logf good to E ulps '''
    a, ea, se, B, S = np.abs(spk['a']), spk['ea'], spk['se'], spk['B'], spk['S']
    rel_se = (ea * (a + 2. * E)).sum(axis=1, keepdims=True) / se + S
    lse = np.log(se)
    err_ce = U32 * (rel_se + 2. * E * np.abs(lse) + np.abs(spk['mx'] + lse))[:, 0] + U32 * np.abs(spk['ce']) + S * TINY
    t0 = spk['w'] / B * (err_ce.sum() + (K_ce + 2) * U32 * np.abs(spk['ce']).sum())
    ps = ea / se
    d = spk['gs'] * spk['w'] / B * U32 * (ps * (a + 2. * E + rel_se + 1.) + 4. * (ps + spk['onehot'])) + TINY
    return t0, d


def spk_sensitivity(spk):
    ''' what ONE ulp of expf / logf moves terms[0] and d_spk by: spk_bounds is linear in E '''
    t1, d1 = spk_bounds(spk, 0, 1.)
    t0, d0 = spk_bounds(spk, 0, 0.)
    return t1 - t0, d1 - d0


GRAD_ROUNDINGS = {'d_dur': 6, 'd_energy': 6, 'd_pitch': 6, 'd_mel': 8}


def grad_bound(name, g):
    return GRAD_ROUNDINGS[name] * U32 * np.abs(g) * (1. + 16 * U32)


def post_grad_bound(g, old, K_post):
    return (K_post + 5) * U32 * np.abs(g) + U32 * (np.abs(old) + np.abs(g))


# ---------------------------------------------------------------------------------------------------- Adam
def step_scalars(lr, betas, t):
    ''' (lr, bc1, bc2_sqrt) as dx_step_scalars_set leaves them in the step block, and as dx_adam_step forms them by value '''
    b1, b2 = f32(betas[0]), f32(betas[1])
    return f32(lr), f32(1. - b1 ** t), f32(math.sqrt(1. - b2 ** t))


AdamResult = namedtuple('AdamResult', 'p m v gsq ep em ev coef')


def adam(p, g, m, v, lr, betas, eps, wd, t, clip=math.inf, gnorm_sq=None, scalars=None):
    ''' one step of torch.optim.Adam (coupled L2, amsgrad off) behind clip_grad_norm_, on float64 copies of the fp32 inputs.
        gnorm_sq: the sum of squares the clipping uses (an input: the GPU test passes the device's own fp32 value);
        scalars: (lr, bc1, bc2_sqrt) of a step block, which then replace lr and t.  Returns p, m, v, sum(g^2) and the bounds. '''
    p, g, m, v = [np.asarray(x, dtype=np.float64) for x in (p, g, m, v)]
    b1, b2, eps, wd, clip = f32(betas[0]), f32(betas[1]), f32(eps), f32(wd), f32(clip)
    lr, bc1, bc2s = scalars if scalars is not None else step_scalars(lr, betas, t)
    coef = 1.
    if gnorm_sq is not None and clip < math.inf:
        coef = min(1., clip / (math.sqrt(float(gnorm_sq)) + f32(1e-6)))
    step = lr / bc1
    gi = g * coef + wd * p
    m1 = b1 * m + (1. - b1) * gi
    v1 = b2 * v + (1. - b2) * gi * gi
    r = np.sqrt(v1)
    D = r / bc2s + eps
    upd = step * m1 / D
    p1 = p - upd
    G = np.abs(g * coef) + np.abs(wd * p)
    em = 8 * U32 * (np.abs(b1 * m) + (1. - b1) * G)
    ev = 14 * U32 * (b2 * v + (1. - b2) * G * G)
    with np.errstate(divide='ignore', invalid='ignore'):
        er = np.where(r > 0, np.minimum(ev / (2. * r), np.sqrt(ev)), np.sqrt(ev)) + U32 * r
    eD = (er + U32 * r) / bc2s + U32 * D
    eU = 3 * U32 * np.abs(upd) + step * em / D + np.abs(upd) * eD / (D - eD)
    ep = eU + U32 * (np.abs(p) + np.abs(upd))
    return AdamResult(p1, m1, v1, float((g * g).sum()), ep, em, ev, coef)


# ---------------------------------------------------------------------------------------------------- the operand copies
def frag_order(src):
    ''' dx_pack_frag_major of an index array src [3][R][K] (R, K multiples of 32), as its comment in conv_pack.hip states it:
        out[chunk][tap][half][block][lane][8] = src[tap][32 block + (lane & 31)][32 chunk + 16 half + 8 (lane >> 5) + 0..7] '''
    taps, R, K = src.shape
    assert taps == 3 and R % 32 == 0 and K % 32 == 0
    chunk, tap, half, block, lane, e = np.meshgrid(np.arange(K // 32), np.arange(3), np.arange(2), np.arange(R // 32), np.arange(64),
                                                   np.arange(8), indexing='ij')
    return src[tap, 32 * block + (lane & 31), 32 * chunk + 16 * half + 8 * (lane >> 5) + e].reshape(-1)


def pack_layouts(p, Cout, Cin, taps):
    ''' flat index arrays (into the parameter buffer) of the copies of the weight (Cout, Cin, taps) at offset p:
        fwd[tap][co][ci], tr[taps - 1 - tap][ci][co] and, where they exist, the fragment-order copies of both '''
    idx = p + np.arange(Cout * Cin * taps, dtype=np.int64).reshape(Cout, Cin, taps)
    fwd = np.empty((taps, Cout, Cin), dtype=np.int64)
    tr = np.empty((taps, Cin, Cout), dtype=np.int64)
    for tap in range(taps):
        fwd[tap] = idx[:, :, tap]
        tr[taps - 1 - tap] = idx[:, :, tap].T
    out = {'fwd': fwd.reshape(-1), 'tr': tr.reshape(-1)}
    if taps == 3 and Cout % 32 == 0 and Cin % 32 == 0:
        out['frag_fwd'], out['frag_tr'] = frag_order(fwd), frag_order(tr)
    return out


# the synthetic table of the fused-Adam test: (Cout, Cin, taps, fragment copies), flat ranges, and the sentinel gaps between entries
PACK_WEIGHTS = [(64, 32, 3, True), (40, 72, 3, False), (33, 31, 1, False), (32, 32, 1, False)]
PACK_FLATS = [1, 4095, 4096, 4097, 3 * 4096 + 5]
PACK_GAPS = [5, 1, 7, 3, 2, 9, 1, 6, 4, 11]


def pack_plan():
    ''' ([(offset, (Cout, Cin, taps), frag)], [(offset, n)], total, live mask): weights and flat ranges interleaved, a gap in front of
        each entry and behind the last '''
    entries = []
    for i in range(max(len(PACK_WEIGHTS), len(PACK_FLATS))):
        if i < len(PACK_FLATS):
            entries.append(('f', PACK_FLATS[i]))
        if i < len(PACK_WEIGHTS):
            entries.append(('w', PACK_WEIGHTS[i]))
    off, ws, fs = 0, [], []
    for (kind, e), gap in zip(entries, PACK_GAPS):
        off += gap
        if kind == 'w':
            ws.append((off, e[:3], e[3]))
            off += e[0] * e[1] * e[2]
        else:
            fs.append((off, e))
            off += e
    total = off + PACK_GAPS[len(entries)]
    live = np.zeros(total, dtype=bool)
    for o, (co, ci, t), _ in ws:
        live[o:o + co * ci * t] = True
    for o, n in fs:
        live[o:o + n] = True
    return ws, fs, total, live


# ---------------------------------------------------------------------------------------------------- sizes of the other GPU cases
SUMSQ_SMALL = (0, 1, 3, 4, 5, 1023, 1024, 2049)
# capped grid, stride s = 1024 * 256 quads; 7 s + 37 quads: every thread makes one unrolled trip, threads 0..36 a second one whose
# last quad is nq - 1 (thread 37 is the first that must NOT: `<=` for `<` would send it one quad past the end), the others three
# remainder trips; two more floats, so that three of the four pointer offsets leave a tail
SUMSQ_BIG = 4 * (7 * SUMSQ_GRID_CAP * BLOCK + 37) + 2
ADAM_SIZES = (1, 255, 256, 257, 70001)
