"""The attention kernels (csrc/attention.hip) called directly -- forward, the dQ / dK-dV pair and the fused d_head 16 backward, in
both operand types and all four head sizes -- and compared element by element with the float64 restatement of
tests/attention_oracle.py under the dropout mask that the kernels draw (tests/dropout_masks.attn_keep).

Tolerance, per case, utterance and tensor (o, lse, dq, dk, dv; live rows), computed on the same inputs:
    4 * max|restatement - float64| + 1e-6 * max|float64|                        (absolute)
where the restatement is the float32 one for the fp32 kernels and for lse, and the bf16 operand emulation (fp32 arithmetic, bf16
where the kernels round) for o and the gradients of the bf16 kernels.  tests/test_attention_host.py holds the first term under
2e-5 (fp32, lse) / 8e-2 (bf16) of the tensor's largest element for every case, so no bound can go slack.  dq and dk of a one-key
utterance are zero by construction and get attention_oracle.cancellation_floor on top.  The bf16 bounds see errors of about a
percent of a tensor's maximum; the fp32 instantiations of the same templates carry the sharp statement for the index, mask and
reduction logic, and the mask readout pins the mask of every kernel -- the fused one has no fp32 form -- to the integer counts
of the numpy restatement.

Cases (E = 128; every one in fp32 and bf16, at p = 0.1 and p = 0, A also at p = 0.5):
    A  N 150, lens 150 97 33            generic; N % 4 = 2: the last 4 x 4 dropout block is partial.  Also at E = 64 and E = 256 (H = 4)
    B  N 259, twelve lens 259 ... 1 0   both sides of the 32-key block and of the 128-row stage, one key, an empty utterance, B > 8
    C  N 1024, lens 1024 513 512 545 1  fused kernel: one workgroup at 512, two at 513 (8 + 9 key blocks), 545 (9 + 9) and 1024
    D  N 1030, lens 1030 515            N > 1024: ATTN_AUTO takes the two-pass pair, ATTN_FUSED is refused
    E  N 300, lens 300 252 3            fill_end = 257 < N: rows of NaN exist
    F  N 70, 19 lens in 0..70           three XCD groups of attn_decode, the odd one reversed, a grid rounded up to 24; with and without length_order
    G  N 300, lens 300 129 64           qkv * 4 and scores that grow with the key index: the alpha rescale, and the merge of the wave groups for d_head >= 64
A, B, E, G at H = 8, 4, 2, 1 (d_head 16, 32, 64, 128); C, D, F at H = 8 and 2.

Measured on an MI355X, kernel error / bound: the worst ratio of a case over its utterances, tensors (o | lse | dq, dk, dv) and
dropout rates, and the median over all of them (d_head 16 and 64 of case A include the E = 64 and E = 256 runs):
    kernel    type  d_head    A     B     C     D     E     F     G   median
    fwd o     fp32    16    0.16  0.31  0.58  0.58  0.29  0.24  0.26    0.25
    fwd o     fp32    32    0.17  0.29     -     -  0.39     -  0.26    0.26
    fwd o     fp32    64    0.18  0.19  0.32  0.30  0.24  0.19  0.20    0.18
    fwd o     fp32   128    0.17  0.16     -     -  0.17     -  0.22    0.16
    fwd o     bf16    16    0.34  0.28  0.33  0.25  0.27  0.27  0.25    0.25
    fwd o     bf16    32    0.27  0.29     -     -  0.26     -  0.26    0.26
    fwd o     bf16    64    0.29  0.27  0.28  0.27  0.27  0.32  0.27    0.27
    fwd o     bf16   128    0.27  0.27     -     -  0.26     -  0.31    0.26
    fwd lse   fp32    16    0.13  0.11  0.13  0.14  0.12  0.13  0.14    0.13
    fwd lse   fp32    32    0.11  0.12     -     -  0.11     -  0.10    0.11
    fwd lse   fp32    64    0.12  0.12  0.13  0.13  0.11  0.12  0.13    0.12
    fwd lse   fp32   128    0.08  0.15     -     -  0.16     -  0.16    0.15
    fwd lse   bf16    16    0.12  0.14  0.14  0.14  0.11  0.13  0.06    0.12
    fwd lse   bf16    32    0.10  0.12     -     -  0.11     -  0.09    0.10
    fwd lse   bf16    64    0.12  0.11  0.13  0.13  0.10  0.12  0.08    0.12
    fwd lse   bf16   128    0.10  0.11     -     -  0.11     -  0.06    0.10
    two-pass  fp32    16    0.39  0.52  0.63  0.75  0.48  0.47  0.47    0.34
    two-pass  fp32    32    0.35  0.51     -     -  0.41     -  0.42    0.32
    two-pass  fp32    64    0.31  0.48  0.53  0.56  0.31  0.31  0.33    0.29
    two-pass  fp32   128    0.23  0.42     -     -  0.38     -  0.46    0.26
    two-pass  bf16    16    0.26  0.47  0.28  0.26  0.25  0.30  0.28    0.25
    two-pass  bf16    32    0.28  0.35     -     -  0.30     -  0.25    0.25
    two-pass  bf16    64    0.31  0.34  0.29  0.27  0.25  0.35  0.49    0.25
    two-pass  bf16   128    0.29  0.31     -     -  0.27     -  0.36    0.25
    fused     bf16    16    0.26  0.47  0.28     -  0.25  0.30  0.28    0.25
The largest ratio anywhere is 0.75 (fp32 d_head 16, dv of case D, N = 1030); summation order did not have to be matched.  A
ratio of exactly 0.25 means that the kernel's largest error is the emulation's own: the same bf16 rounding of the same element.
Mask readout: every count exact; off-integer part 0.000 in fp32 and at most 0.211 in bf16 (o, 1024 keys, 64 per class; dq 0.034).
The 294 tests take 8 s together, the slowest (case C, H = 8: the numpy mask of 5 x 8 x 1024 x 1024) half a second.
"""
import functools
import types

import pytest
import torch

from tests import attention_oracle as A
from tests.util import fill_end

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32, BF16 = torch.float32, torch.bfloat16
NAME = {F32: 'fp32', BF16: 'bf16'}


def _configs():
    out = []
    for name in A.CASES:
        shapes = [(H, 128) for H in A.HEADS[name]] + ([(4, 64), (4, 256)] if name == 'A' else [])
        for H, E in shapes:
            for dtype in (F32, BF16):
                for p in ((0.1, 0., 0.5) if name == 'A' else (0.1, 0.)):
                    for ordered in ((False, True) if name == 'F' else (False,)):
                        cfg = (name, H, E, dtype, p, ordered)
                        out.append(pytest.param(cfg, id=f'{name}-H{H}-E{E}-{NAME[dtype]}-p{p}' + ('-ordered' if ordered else '')))
    return out


CONFIGS = _configs()


def _can_fuse(cfg):
    name, H, E, dtype, p, ordered = cfg
    return dtype == BF16 and E // H == 16 and A.CASES[name][0] <= 1024


def _counters(c):
    from daft_exprt import ops
    B, N = c.d_o.shape[:2]
    return ops._attn_workspace(B, N, c.H, c.qkv.device)


def _backward(c, algo, qkv=None, d_o=None, lens=None, o=None, lse=None, order=None):
    ''' one call of ops.attention_bwd on the case's tensors (or the given ones); the arrival counters must be back at zero after it '''
    from daft_exprt import ops
    pick = lambda given, own: own if given is None else given
    dqkv = ops.attention_bwd(pick(qkv, c.qkv), pick(o, c.o), pick(d_o, c.d_o), pick(lse, c.lse), pick(lens, c.lens), c.H, c.p, A.SEED,
                             order=pick(order, c.order), algo=algo)
    assert not bool(_counters(c)[1].any()), 'arrival counters must be zero after every backward call'
    return dqkv


def _forward(c, qkv=None, lens=None, order=None):
    from daft_exprt import ops
    pick = lambda given, own: own if given is None else given
    return ops.attention_fwd(pick(qkv, c.qkv), pick(lens, c.lens), c.H, c.p, A.SEED, order=pick(order, c.order))


@functools.lru_cache(maxsize=None)
def _case(cfg):
    ''' inputs, the float64 reference, the restatements and one forward run of a configuration, shared by the tests and left unchanged;
        the backward of an algorithm is run on first use (`_grads`) '''
    from daft_exprt import ops
    name, H, E, dtype, p, ordered = cfg
    c = types.SimpleNamespace(name=name, H=H, E=E, dtype=dtype, p=p)
    qkv, d_o, lens = A.make_case(name, H, dtype, E)
    c.B, c.N = d_o.shape[:2]
    c.lens_list = lens.tolist()
    keep, c.scale = A.keep_of(c.B, H, c.N, p)
    c.cpu = (qkv, d_o, lens)
    c.ref = A.reference(qkv, d_o, lens, H, keep, c.scale, torch.float64)
    c.low = {'fp32': A.reference(qkv, d_o, lens, H, keep, c.scale, torch.float32)}
    if dtype == BF16:
        c.low['bf16'] = A.emulate_bf16(qkv, d_o, lens, H, keep, c.scale)
    c.qkv, c.d_o, c.lens = qkv.to(DEV), d_o.to(DEV), lens.to(DEV)
    c.order = ops.length_order(c.lens) if ordered else None
    c.o, c.lse = _forward(c)
    c.fe = fill_end(lens, c.N).tolist()
    c.grads = {}
    torch.cuda.synchronize()
    return c


def _grads(c, algo):
    if algo not in c.grads:
        c.grads[algo] = _backward(c, algo)
    return c.grads[algo]


def _check(c, got, label):
    ''' every tensor of `got` within its bound of the float64 reference, per utterance, on live rows; prints the worst
        error / bound ratio per tensor and asserts after printing '''
    bad, worst = [], {}
    qkv, d_o, lens = c.cpu
    for t, g in got.items():
        g = g.double().cpu()
        for b, n in enumerate(c.lens_list):
            if n == 0:
                continue
            bnd, _ = A.bound(c.low[A.restatement_of(t, c.dtype)], c.ref, t, b, n)
            bnd += A.cancellation_floor(qkv, d_o, lens, c.H, c.scale, b, t)
            err = float((A.live(g, t, b, n) - A.live(c.ref[t], t, b, n)).abs().max())
            ratio = err / bnd if bnd > 0. else (0. if err == 0. else float('inf'))
            worst[t] = max(worst.get(t, 0.), ratio)
            if not err <= bnd:
                bad.append((t, b, n, err, bnd))
    print(f'RATIO {label} {c.name} H{c.H} E{c.E} {NAME[c.dtype]} p{c.p}:', ' '.join(f'{t} {r:.3f}' for t, r in worst.items()))
    assert not bad, (label, c.name, c.H, c.E, c.dtype, c.p, bad)


def _split(c, dqkv):
    dq, dk, dv = dqkv.split(c.E, dim=2)
    return {'dq': dq, 'dk': dk, 'dv': dv}


def _check_dead_rows(c, dqkv):
    ''' rows len <= n < fill_end of dqkv are exactly zero (dx_common.h); nothing is said about the rows from fill_end on '''
    for b, (n, fe) in enumerate(zip(c.lens_list, c.fe)):
        assert not bool(dqkv[b, n:fe].any()), (c.name, b, 'dead rows of dqkv below the fill end must be exactly zero')


@pytest.mark.parametrize('cfg', CONFIGS)
def test_forward(cfg):
    c = _case(cfg)
    assert c.o.dtype == c.dtype and c.lse.dtype == torch.float32
    _check(c, {'o': c.o, 'lse': c.lse}, 'fwd')
    for b, (n, fe) in enumerate(zip(c.lens_list, c.fe)):
        assert bool(torch.isfinite(c.o[b, n:fe]).all()), (c.name, b, 'o below the fill end must be finite')


@pytest.mark.parametrize('cfg', CONFIGS)
def test_backward_two_pass(cfg):
    from daft_exprt import ops
    c = _case(cfg)
    dqkv = _grads(c, ops.ATTN_TWO_PASS)
    _check(c, _split(c, dqkv), 'two_pass')
    _check_dead_rows(c, dqkv)


@pytest.mark.parametrize('cfg', [p for p in CONFIGS if _can_fuse(p.values[0])])
def test_backward_fused(cfg):
    from daft_exprt import ops
    c = _case(cfg)
    dqkv = _grads(c, ops.ATTN_FUSED)
    _check(c, _split(c, dqkv), 'fused')
    _check_dead_rows(c, dqkv)
    assert _same_bits(c, dqkv, _grads(c, ops.ATTN_AUTO), 'fill'), 'ATTN_AUTO must take the fused kernel here'


@pytest.mark.parametrize('cfg', [p for p in CONFIGS if p.values[0][0] == 'D'])
def test_backward_auto_takes_the_two_pass_pair_past_1024(cfg):
    from daft_exprt import ops
    c = _case(cfg)
    dqkv = _grads(c, ops.ATTN_AUTO)
    _check(c, _split(c, dqkv), 'auto')
    _check_dead_rows(c, dqkv)
    assert _same_bits(c, dqkv, _grads(c, ops.ATTN_TWO_PASS), 'fill')


# ----------------------------------------------------------------------------- mask readout
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('H', [8, 2])
@pytest.mark.parametrize('N,lens', [(512, [512, 64]), (1024, [1024])])
def test_mask_readout(N, lens, H, dtype):
    ''' q = 0 and one-hot v / d_o (k for the dq pattern): o, dv and dq hold integer counts of kept keys / kept queries per class, which
        must be those of attn_keep exactly -- for the forward, the dQ kernel, the dK/dV kernel and the fused one, whatever the
        operand precision '''
    from daft_exprt import ops
    keep, scale = A.keep_of(len(lens), H, N, 0.1)
    algos = [ops.ATTN_TWO_PASS] + ([ops.ATTN_FUSED] if (dtype == BF16 and H == 8) else [])
    for pattern in (0, 1, 2):
        want_o, want_dv = A.readout_counts(keep, lens, H, pattern % 2)
        qkv, d_o, lengths = (t.to(DEV) for t in A.readout_inputs(N, lens, H, dtype, pattern))
        o, lse = ops.attention_fwd(qkv, lengths, H, 0.1, A.SEED)
        got = [('o', A.decode_counts(o, lens, scale).cpu(), want_o)] if pattern < 2 else []
        for algo in algos:
            dqkv = ops.attention_bwd(qkv, o, d_o, lse, lengths, H, 0.1, A.SEED, algo=algo)
            if pattern < 2:
                got.append((f'dv algo {algo}', A.decode_counts(dqkv[:, :, 2 * 128:], lens, scale).cpu(), want_dv))
            else:
                got.append((f'dq algo {algo}', A.decode_dq_counts(dqkv[:, :, :128], o, lens, H, scale).cpu(), want_o))
        for label, counts, want in got:
            off = float((counts - counts.round()).abs().max())
            wrong = int((counts.round().long() != want).sum())
            print(f'READOUT N{N} H{H} {NAME[dtype]} pattern {pattern} {label}: off-integer {off:.3f}, wrong counts {wrong}')
            assert off <= 0.25 and wrong == 0, (label, pattern, off, wrong)


# ----------------------------------------------------------------------------- contracts
def _same_bits(c, a, b, rows, lens=None):
    ''' a and b, (B, N, C) or the (B, H, N) lse, hold the same bits on the live rows (`rows` = 'live') or below the fill end ('fill') '''
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.shape[1] == c.H and a.shape[2] == c.N:          # lse
        a, b = a.transpose(1, 2), b.transpose(1, 2)
    as_int = torch.int32 if a.dtype == torch.float32 else torch.int16
    lens = c.lens_list if lens is None else lens
    ends = lens if rows == 'live' else fill_end(lens, c.N).tolist()
    return all(torch.equal(a[i, :e].contiguous().view(as_int), b[i, :e].contiguous().view(as_int)) for i, e in enumerate(ends))


def _algos(cfg):
    from daft_exprt import ops
    return [ops.ATTN_TWO_PASS] + ([ops.ATTN_FUSED] if _can_fuse(cfg) else [])


CONTRACT_SHAPES = [(H, dtype) for H in (8, 2) for dtype in (F32, BF16)]
CONTRACT_IDS = [f'H{H}-{NAME[dtype]}' for H, dtype in CONTRACT_SHAPES]


@pytest.mark.parametrize('H,dtype', CONTRACT_SHAPES, ids=CONTRACT_IDS)
@pytest.mark.parametrize('name', ['B', 'E'])
def test_live_rows_do_not_depend_on_the_padding(name, H, dtype):
    ''' zeros for the finite garbage below the fill end and other values for the NaN past it: the live rows keep their bits '''
    cfg = (name, H, 128, dtype, 0.1, False)
    c = _case(cfg)
    qkv, d_o = c.qkv.clone(), c.d_o.clone()
    for b, (n, fe) in enumerate(zip(c.lens_list, c.fe)):
        qkv[b, n:fe], d_o[b, n:fe] = 0., 0.
        qkv[b, fe:], d_o[b, fe:] = 3., -5.
    o, lse = _forward(c, qkv=qkv)
    assert _same_bits(c, o, c.o, 'live') and _same_bits(c, lse, c.lse, 'live')
    for algo in _algos(cfg):
        assert _same_bits(c, _backward(c, algo, qkv=qkv, d_o=d_o), _grads(c, algo), 'live'), algo


@pytest.mark.parametrize('cfg,algo', [(('C', 8, 128, BF16, 0.1, False), 2), (('A', 8, 128, BF16, 0.1, False), 1), (('A', 8, 128, F32, 0.1, False), 1),
                                      (('A', 2, 128, BF16, 0.1, False), 1)], ids=['C-fused', 'A-two_pass-bf16', 'A-two_pass-fp32', 'A-two_pass-bf16-H2'])
def test_backward_reads_nothing_from_its_workspace_that_it_did_not_write(cfg, algo):
    c = _case(cfg)
    first = _grads(c, algo)
    ws, counters = _counters(c)
    ws.fill_(float('nan'))
    assert _same_bits(c, _backward(c, algo), first, 'fill')


@pytest.mark.parametrize('H,dtype', CONTRACT_SHAPES, ids=CONTRACT_IDS)
def test_calls_are_reproducible_and_the_launch_order_changes_no_bit(H, dtype):
    from daft_exprt import ops
    cfg = ('F', H, 128, dtype, 0.1, False)
    c = _case(cfg)
    order = ops.length_order(c.lens)
    by_length = sorted(range(c.B), key=lambda i: (-c.lens_list[i], i))
    assert order.tolist() == by_length
    for kw in ({}, {'order': order}):
        o, lse = _forward(c, **kw)
        assert _same_bits(c, o, c.o, 'live') and _same_bits(c, lse, c.lse, 'live'), kw
        for algo in _algos(cfg):
            assert _same_bits(c, _backward(c, algo, **kw), _grads(c, algo), 'fill'), (algo, kw)


@pytest.mark.parametrize('H,dtype', CONTRACT_SHAPES, ids=CONTRACT_IDS)
@pytest.mark.parametrize('p', [0., 0.1])
def test_an_utterance_does_not_depend_on_its_batch(p, H, dtype):
    ''' utterance b run alone at the same N gives the bits it has in the batch (p = 0); the dropout mask depends on b, so with
        p > 0 only utterance 0 can be compared '''
    cfg = ('B', H, 128, dtype, p, False)
    c = _case(cfg)
    for b in (range(c.B) if p == 0. else [0]):
        one = dict(qkv=c.qkv[b:b + 1].contiguous(), lens=c.lens[b:b + 1].contiguous())
        alone = types.SimpleNamespace(H=c.H, N=c.N, lens_list=c.lens_list[b:b + 1])
        o, lse = _forward(c, **one)
        assert _same_bits(alone, o, c.o[b:b + 1], 'live') and _same_bits(alone, lse, c.lse[b:b + 1], 'live'), b
        for algo in _algos(cfg):
            dqkv = _backward(c, algo, d_o=c.d_o[b:b + 1].contiguous(), o=o, lse=lse, **one)
            assert _same_bits(alone, dqkv, _grads(c, algo)[b:b + 1], 'live'), (b, algo)


@pytest.mark.parametrize('cfg', [('A', 8, 128, F32, 0.1, False), ('A', 2, 128, BF16, 0.1, False), ('A', 4, 128, BF16, 0.1, False),
                                 ('D', 8, 128, BF16, 0.1, False)], ids=['fp32', 'd_head64', 'd_head32', 'N1030'])
def test_fused_backward_is_refused_where_it_does_not_apply(cfg):
    from daft_exprt import ops
    c = _case(cfg)
    with pytest.raises(RuntimeError, match='fused kernel'):
        _backward(c, ops.ATTN_FUSED)
