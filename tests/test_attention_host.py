"""tests/attention_oracle.py checked on the CPU: its closed-form backward against autograd, its forward against torch's own
attention, and the two conditions on the INPUTS of tests/test_gpu_attention.py -- the low-precision restatements stay within
the cap (so no bound of that file can go slack), and the mask readout separates adjacent counts."""
import math

import pytest
import torch

from tests import attention_oracle as A

P_OF = {name: ((0.1, 0.) if name != 'A' else (0.1, 0., 0.5)) for name in A.CASES}
CONFIGS = [(name, H, 128) for name in A.CASES for H in A.HEADS[name]] + [('A', 4, 64), ('A', 4, 256)]


def _small():
    qkv, d_o, lens = A.make_case('A', 8, torch.float32)
    return qkv[:, :40].contiguous(), d_o[:, :40].contiguous(), torch.tensor([40, 33, 7])


@pytest.mark.parametrize('p', [0., 0.1, 0.5])
@pytest.mark.parametrize('H', [8, 2])
def test_closed_form_backward_equals_autograd(p, H):
    qkv, d_o, lens = _small()
    keep, scale = A.keep_of(3, H, 40, p)
    ref = A.reference(qkv, d_o, lens, H, keep, scale, torch.float64)
    x = qkv.double().requires_grad_(True)
    o, lse = A.forward(x, lens, H, keep, scale, torch.float64)
    liv = (torch.arange(40)[None, :] < lens[:, None]).unsqueeze(2)
    (o * d_o.double() * liv).sum().backward()
    E = 128
    assert torch.equal(o.detach(), ref['o'])
    for name, got in zip(('dq', 'dk', 'dv'), x.grad.split(E, dim=2)):
        err = float((got * liv - ref[name]).abs().max())
        assert err <= 1e-12 * max(1., float(ref[name].abs().max())), (name, err)
        assert float(ref[name].abs().max()) > 0.1


@pytest.mark.parametrize('name,H', [('A', 8), ('A', 1), ('E', 2), ('B', 4)])
def test_reference_without_dropout_equals_scaled_dot_product_attention(name, H):
    ''' the independent restatement sees the whole padded batch and a key mask; the reference cuts every utterance to its live rows '''
    qkv, d_o, lens = A.make_case(name, H, torch.float32)
    B, N, E = d_o.shape
    ref = A.reference(qkv, d_o, lens, H, None, 1., torch.float64)
    x = torch.nan_to_num(qkv.double(), nan=0.)
    q, k, v = (t.reshape(B, N, H, E // H).transpose(1, 2) for t in x.split(E, dim=2))
    pad = torch.arange(N)[None, :] >= lens[:, None]
    mask = (~pad)[:, None, None, :] | (lens == 0)[:, None, None, None]         # (an empty utterance: keep its unused softmax finite)
    sdpa = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2).reshape(B, N, E)
    s = (q @ k.transpose(2, 3)) / math.sqrt(E // H)
    lse = torch.logsumexp(s.masked_fill(~mask, float('-inf')), dim=3)
    for b, n in enumerate(lens.tolist()):
        assert float((sdpa[b, :n] - ref['o'][b, :n]).abs().max() if n else 0.) <= 1e-12
        assert float((lse[b, :, :n] - ref['lse'][b, :, :n]).abs().max() if n else 0.) <= 1e-12
        assert not ref['o'][b, n:].any() and not ref['dq'][b, n:].any()


@pytest.mark.parametrize('name,H,E', CONFIGS)
def test_restatements_stay_within_the_cap(name, H, E):
    ''' 4 * max|restatement - float64| <= CAP * max|float64| per utterance and tensor, for both operand types and every dropout
        rate the GPU test uses.  Not asked of dq / dk of a one-key utterance: they are zero by construction (see
        attention_oracle.cancellation_floor) and hold cancellation noise only. '''
    worst = {}
    for dtype in (torch.float32, torch.bfloat16):
        qkv, d_o, lens = A.make_case(name, H, dtype, E)
        B, N = d_o.shape[:2]
        for p in P_OF[name]:
            keep, scale = A.keep_of(B, H, N, p)
            ref = A.reference(qkv, d_o, lens, H, keep, scale, torch.float64)
            low = {'fp32': A.reference(qkv, d_o, lens, H, keep, scale, torch.float32)}
            if dtype == torch.bfloat16:
                low['bf16'] = A.emulate_bf16(qkv, d_o, lens, H, keep, scale)
            for b, n in enumerate(lens.tolist()):
                for t in A.TENSORS:
                    if n == 0 or (n == 1 and t in ('dq', 'dk')):
                        continue
                    which = A.restatement_of(t, dtype)
                    _, frac = A.bound(low[which], ref, t, b, n)
                    cap = A.CAP[torch.bfloat16 if which == 'bf16' else torch.float32]
                    key = (str(dtype)[6:], which, t)
                    worst[key] = max(worst.get(key, 0.), frac / cap)
                    assert frac <= cap, ('restatement too far from float64: change the inputs', name, H, E, dtype, p, b, t, frac)
                    assert float(A.live(ref[t], t, b, n).abs().max()) > 0. or n == 1
    print(name, H, E, ' '.join(f'{k[0]}/{k[2]}:{v:.2f}' for k, v in sorted(worst.items())))


@pytest.mark.parametrize('H', [8, 2])
@pytest.mark.parametrize('N,lens', [(512, [512, 64]), (1024, [1024])])
def test_mask_readout_decodes_integer_counts(N, lens, H):
    ''' with the reference standing in for the kernel, in both operand types and for the three input patterns: every decoded count is
        within 0.25 of an integer, and that integer is the count of attn_keep '''
    keep, scale = A.keep_of(len(lens), H, N, 0.1)
    stand_in = lambda inp, dtype: (A.emulate_bf16(*inp, H, keep, scale) if dtype == torch.bfloat16 else
                                   A.reference(*inp, H, keep, scale, torch.float32))
    for pattern in (0, 1):
        want_o, want_dv = A.readout_counts(keep, lens, H, pattern)
        for dtype in (torch.float32, torch.bfloat16):
            got = stand_in(A.readout_inputs(N, lens, H, dtype, pattern), dtype)
            for t, want in (('o', want_o), ('dv', want_dv)):
                counts = A.decode_counts(got[t], lens, scale)
                assert float((counts - counts.round()).abs().max()) <= 0.25, (dtype, t, pattern)
                assert torch.equal(counts.round().long(), want), (dtype, t, pattern)
        for want in (want_o, want_dv):          # the mask really drops, and differently from row to row
            per_row = want[0, :lens[0], :128 // H].sum(dim=1)
            assert int(per_row.min()) < int(per_row.max()) < lens[0]
    want_o = A.readout_counts(keep, lens, H, 0)[0]
    for dtype in (torch.float32, torch.bfloat16):          # the dq pattern
        got = stand_in(A.readout_inputs(N, lens, H, dtype, 2), dtype)
        counts = A.decode_dq_counts(got['dq'], got['o'], lens, H, scale)
        assert float((counts - counts.round()).abs().max()) <= 0.25, dtype
        assert torch.equal(counts.round().long(), want_o), dtype
