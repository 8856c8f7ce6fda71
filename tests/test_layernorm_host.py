"""tests/layernorm_oracle.py checked on the CPU: its closed-form backward against float64 autograd of its own forward, its forward
against torch's layer_norm, and the two conditions on the INPUTS of tests/test_gpu_layernorm.py -- the low-precision
restatement stays within the cap (so no bound of that file can go slack), and the mask readout separates kept from dropped."""
import pytest
import torch

from tests import dropout_masks as DM
from tests import layernorm_oracle as L

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DROPOUTS = ((0., 0.), (0.1, 0.), (0., 0.3), (0.2, 0.3))


def _autograd(c):
    ''' float64 autograd of the oracle's forward: d(sum y * dy over the rows where y is not masked) / d(x, residual, gamma, beta, film) '''
    leaf = lambda t: None if t is None else t.double().masked_fill(~torch.isfinite(t.double()), 0.).requires_grad_(True)
    x, res, gamma, beta, film = leaf(c.x), leaf(c.residual), leaf(c.gamma), leaf(c.beta), leaf(c.film)
    if c.relu:
        y = L.forward(c, F64, torch.relu(x), res, gamma, beta, film)[0]       # c.x = relu(c.x) already: relu(x) is x, and its derivative the gate
    else:
        y = L.forward(c, F64, x, res, gamma, beta, film)[0]
    gy = c.dy.double().masked_fill(~(c.live & c.comp)[:, :, None], 0.)
    (y * gy).sum().backward()
    return x.grad, (None if res is None else res.grad), gamma.grad, beta.grad, (None if film is None else film.grad)


OPTIONS = [(name, variant, residual, film, pp) for name in ('A', 'B', 'D', 'E') for variant in L.VARIANTS[name]
           for residual, film in ((True, True), (False, False), (True, False), (False, True)) for pp in DROPOUTS
           if not (name == 'E' and residual)]


@pytest.mark.parametrize('name,variant,residual,film,pp', OPTIONS)
def test_closed_form_backward_equals_autograd(name, variant, residual, film, pp):
    ''' every option combination of the GPU file: residual, FiLM, both dropouts, lengths, the three skip forms, and (case E) the
        ReLU gate -- there x = relu(x) enters the forward through a relu, whose derivative is the gate of ds '''
    c = L.make_case(name, 128, variant, residual=residual, film=film, p_pre=pp[0], p_post=pp[1])
    ref = L.reference(c)
    dx, dres, dgamma, dbeta, dfilm = _autograd(c)
    close = lambda got, want: float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    if c.relu:
        # autograd gates the whole chain behind relu(x): that is dx_pre (= ds, gated) -- the kernel's gate
        assert close(dx, ref['dx_pre'])
        assert bool((ref['ds'][c.x.double().expand_as(ref['ds']) <= 0.] == 0.).all())
    else:
        assert close(dx, ref['dx_pre'])
        if dres is not None:
            assert close(dres, ref['ds'])
        elif pp[0] == 0.:
            assert torch.equal(ref['ds'], ref['dx_pre'])
    assert close(dgamma, ref['dgamma'] - c.init[0].double())
    assert close(dbeta, ref['dbeta'] - c.init[1].double())
    if film:
        assert close(dfilm, ref['dfilm'] - c.init[2].double())
    for t in ('ds', 'dx_pre', 'dgamma', 'dbeta'):
        assert float(ref[t].abs().max()) > 0.1 and bool(torch.isfinite(ref[t]).all())
    if pp[0] > 0.:
        keep, scale = L.keep_of(c, 0)
        assert torch.equal(ref['dx_pre'], ref['ds'] * keep * scale)


def test_the_relu_gate_is_taken_on_s_and_on_ds_alone():
    ''' ds of the gated case = ds of the ungated one with the elements of s <= 0 set to zero; the per-channel sums do not change '''
    c = L.make_case('E', 128, None, residual=False, film=True, p_post=0.3, s_given=True)
    gated = L.reference(c)
    c.relu = False
    plain = L.reference(c)
    zero = c.x.double() <= 0.
    assert 0.3 < float(zero.double().mean()) < 0.7
    assert torch.equal(gated['ds'], plain['ds'].masked_fill(zero, 0.))
    for t in ('dgamma', 'dbeta', 'dfilm'):
        assert torch.equal(gated[t], plain[t])


@pytest.mark.parametrize('name,C', [('A', 128), ('D', 1024), ('B', 512)])
def test_forward_without_options_equals_torch_layer_norm(name, C):
    c = L.make_case(name, C, 'skip_only' if name == 'B' else None, residual=False, film=False)
    c.live = c.comp = torch.ones(c.B, c.N, dtype=torch.bool)
    c.x = torch.nan_to_num(c.x, nan=1.)
    ref = L.reference(c)
    want = torch.nn.functional.layer_norm(c.x.double(), (C,), c.gamma.double(), c.beta.double(), eps=1e-5)
    assert float((ref['y'] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.equal(ref['s'], c.x.double())


CAP_CONFIGS = [(name, C, variant) for name in L.CASES for C in L.WIDTHS[name] for variant in L.VARIANTS[name]]


@pytest.mark.parametrize('name,C,variant', CAP_CONFIGS)
def test_restatements_stay_within_the_cap(name, C, variant):
    ''' max|restatement - float64| <= CAP * max|float64| per utterance and tensor, for both storage types of the inputs and the
        outputs, every dropout setting the GPU test uses, the forward's own statistics and the rounded float64 ones '''
    worst = {'fp32': 0., 'bf16': 0.}
    for x_dtype, dy_dtype, o_dtype in ((F32, F32, F32), (BF16, BF16, BF16), (F32, BF16, BF16)):
        for pp in (DROPOUTS if name != 'C' else DROPOUTS[3:]):
            for s_given in (False, True):
                c = L.make_case(name, C, variant, x_dtype, dy_dtype, p_pre=pp[0], p_post=pp[1], s_given=s_given)
                ref = L.reference(c)
                stats = (ref['mean'].float(), ref['rstd'].float()) if s_given else None
                low = L.restate(c, o_dtype, o_dtype, stats)
                for t in L.FWD_TENSORS + L.BWD_TENSORS:
                    kind = L.restatement_kind(t, o_dtype, o_dtype)
                    for b, fe in L.regions(c, t):
                        if fe == 0:
                            continue
                        _, frac = L.bound(low, ref, t, b, fe)
                        worst[kind] = max(worst[kind], frac)
                        assert frac <= L.CAP[kind], ('restatement too far from float64: change the inputs', name, C, variant, x_dtype, pp, t, b, frac)
    print(f'CAP {name} C{C} {variant}: fp32 {worst["fp32"]:.2e} bf16 {worst["bf16"]:.2e}')
    assert L.CAP['fp32'] <= 2e-5 and L.CAP['bf16'] <= 8e-3


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('C', [128, 1024])
@pytest.mark.parametrize('p', [0.1, 0.5, 0.001])
def test_mask_readout_separates_kept_from_dropped(p, C, dtype):
    ''' with the restatement standing in for the kernel: the four decoded masks are elem_keep's, every kept element of the reference
        is READOUT_MARGIN away from the decision threshold and every dropped one as far on the other side '''
    for stream in (0, 1):
        keep, scale = DM.elem_keep((L.SEED_PRE, L.SEED_POST)[stream], stream, range(L.READOUT_B), L.READOUT_N, C, p)
        keep = torch.from_numpy(keep)
        assert 0 < int((~keep).sum()) < keep.numel() * (p + 0.05)
        c = L.readout_case(C, dtype, p, stream)
        ref, low = L.reference(c), L.restate(c, dtype, dtype)
        assert torch.equal(L.decode_forward(stream, low['y'], low['s']), keep)
        seen = (ref['s'] if stream == 0 else ref['y']).abs()
        assert float(seen[keep].min()) >= L.READOUT_MARGIN and not bool(seen[~keep].any())
        c = L.readout_case(C, dtype, p, stream, s_given=True)
        ref = L.reference(c)
        low = L.restate(c, dtype, dtype, (ref['mean'].float(), ref['rstd'].float()))
        assert torch.equal(L.decode_backward(stream, low['ds'], low['dx_pre'], ref['rstd'], scale), keep)
        if stream == 0:
            assert float(ref['ds'].abs().min()) >= L.READOUT_MARGIN and not bool(ref['dx_pre'][~keep].any())
        else:
            size = ref['ds'].abs() / ref['rstd'][:, :, None]
            assert float(size[keep].min()) >= 2. * scale + L.READOUT_MARGIN and float(size[~keep].max()) <= 2. * scale - L.READOUT_MARGIN
