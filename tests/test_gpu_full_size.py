"""BASELINE configs[1] full size (B = 48, T <= 1000, dropout ON): size-independent properties of the training step.
The CPU oracle needs ~100 s for this batch, so the checks here are internal consistency ones:
  * the fused fast paths (LayerNorm backward inside the data-gradient GEMMs, partial-tile weight gradients) against the
    plain paths (separate LayerNorm-backward launches, fp32 atomics) on the SAME dropout masks: every one of the 193
    gradients must agree to fp32-reordering / bf16-operand precision;
  * a second run of the same step reproduces every prediction bit for bit (no atomics on the forward path) and the loss
    terms / gradients to atomic-reordering precision;
  * scaling the loss gradient scales every parameter gradient (linearity of the hand-written backward)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _setup():
    import bench
    from daft_exprt.data_loader import synthetic_batch
    from daft_exprt.loss import DaftExprtLoss
    from daft_exprt.model import DaftExprt
    hp = bench.make_hparams(48, 'bf16')
    dev = torch.device('cuda:0')
    torch.manual_seed(hp.seed)
    model = DaftExprt(hp).to(dev).train()
    cb = synthetic_batch(hp, 48, seed=1234, t_max=1000, force_first_full=True)
    inputs, targets, _ = model.parse_batch(dev, cb)
    weights = DaftExprtLoss(dev, hp).weights(20000)
    return model, inputs, targets, weights


def _step(model, inputs, targets, weights, step_id, scale=1.):
    model.zero_grad()
    model._step_id = step_id            # same dropout counters for every call
    terms = model.forward_backward(inputs, targets, weights, grad_scale=scale)
    torch.cuda.synchronize()
    return terms.clone(), model._gflat.clone(), [model.last_outputs[3].clone()] + [t.clone() for t in model.last_outputs[2]]


def test_fast_paths_match_plain_paths_and_step_is_reproducible():
    from daft_exprt import ops
    model, inputs, targets, weights = _setup()
    assert int(inputs[9].max()) == 1000 and inputs[0].shape[0] == 48
    t0, g0, o0 = _step(model, inputs, targets, weights, 7)
    t1, g1, o1 = _step(model, inputs, targets, weights, 7)
    assert all(torch.equal(a, b) for a, b in zip(o0, o1))                # mel, durations, energy, pitch: bit-identical
    assert torch.allclose(t0, t1, rtol=1e-5, atol=0.)                    # loss sums: block partials meet in fp32 atomics
    gn = float(g0.norm())
    assert float((g0 - g1).norm()) <= 1e-4 * gn     # per-channel / FiLM atomics reorder, then pass through bf16 GEMM operands
    model.fuse_ln_backward = False
    ops.WGRAD_WORKSPACE = False
    try:
        t2, g2, o2 = _step(model, inputs, targets, weights, 7)
    finally:
        model.fuse_ln_backward = True
        ops.WGRAD_WORKSPACE = True
    assert all(torch.equal(a, b) for a, b in zip(o0, o2)) and torch.allclose(t0, t2, rtol=1e-5, atol=0.)
    assert float((g0 - g2).norm()) <= 1e-3 * gn, float((g0 - g2).norm()) / gn
    # per-parameter: no tensor may hide behind the global norm
    off = 0
    for name, p in model.named_parameters():
        n = p.numel()
        a, b = g0[off:off + n], g2[off:off + n]
        off += n
        assert float((a - b).norm()) <= 1e-2 * float(a.norm()) + 1e-6 * gn, (name, float((a - b).norm()), float(a.norm()))
    # linearity in the loss-gradient scale
    t3, g3, _ = _step(model, inputs, targets, weights, 7, scale=0.5)
    assert float((g3 * 2 - g0).norm()) <= 3e-4 * gn


def test_balanced_tiles_match_fixed_tiles_at_full_size():
    ''' the balanced variable-height tile launches (dx_conv_tile_plan) against the fixed-tile launches on the same dropout
        masks: every prediction bit-identical (same rows, same summation order per output), gradients equal up to the
        order of the per-channel atomics '''
    from daft_exprt import ops
    model, inputs, targets, weights = _setup()
    assert model.balanced_tiles and ops.USE_SPLITK
    ts, gs, os_ = _step(model, inputs, targets, weights, 11)     # default: split-K workgroups on the balanced tiles
    ops.USE_SPLITK = False
    try:
        t0, g0, o0 = _step(model, inputs, targets, weights, 11)  # the ring kernel on the same tiles
        model.balanced_tiles = False
        try:
            t1, g1, o1 = _step(model, inputs, targets, weights, 11)
        finally:
            model.balanced_tiles = True
    finally:
        ops.USE_SPLITK = True
    assert all(torch.equal(a, b) for a, b in zip(o0, o1))
    # split-K adds the two halves of the contraction in another order than the ring kernel's single chain: fp32 rounding of a
    # 3072-term sum in front of bf16 operand roundings -> predictions within a few 1e-3 of the output scale, never bit-equal
    # (end to end the random-init network amplifies such a perturbation ~3.6x per FFT block, see test_gpu_parity_at_size: the mean moves
    # by a few 1e-3 of the output scale, single elements by up to ~15 %)
    for a, b in zip(os_, o0):
        d, scale = (a.float() - b.float()).abs(), max(1., float(b.float().abs().max()))
        assert float(d.mean()) <= 1e-2 * scale and float(d.max()) <= 0.3 * scale, (float(d.mean()), float(d.max()), scale)
    assert float((ts - t0).abs().max()) <= 2e-2 * float(t0.abs().max())
    assert torch.allclose(t0, t1, rtol=1e-5, atol=0.)
    gn = float(g0.norm())
    assert float((g0 - g1).norm()) <= 2e-4 * gn, float((g0 - g1).norm()) / gn


def test_tile_plans_are_rebuilt_for_every_batch():
    ''' two different batches through the same model, back to back: each batch must run on tile plans built from its own
        lengths, never on those of the batch before '''
    import bench
    from daft_exprt.data_loader import synthetic_batch
    from daft_exprt.model import DaftExprt
    hp = bench.make_hparams(48, 'bf16')
    dev = torch.device('cuda:0')
    torch.manual_seed(hp.seed)
    model = DaftExprt(hp).to(dev).eval()
    outs = {}
    for rnd in range(2):
        for seed in (1, 2):
            cb = synthetic_batch(hp, 16, seed=seed, t_max=700, force_first_full=True)
            inputs, _, _ = model.parse_batch(dev, cb)
            with torch.no_grad():
                mel = model(inputs)[3][0].clone()
            del inputs
            if rnd == 0:
                outs[seed] = mel
            else:
                assert torch.equal(outs[seed], mel), seed
    # fixed tiles give the bits of the balanced tiles on the ring kernel (same summation order per output); the split-K kernel adds the
    # two halves of the contraction separately, so it is compared within rounding
    from daft_exprt import ops
    ops.USE_SPLITK = False
    try:
        ring = {}
        for seed in (1, 2):
            cb = synthetic_batch(hp, 16, seed=seed, t_max=700, force_first_full=True)
            inputs, _, _ = model.parse_batch(dev, cb)
            with torch.no_grad():
                ring[seed] = model(inputs)[3][0].clone()
            d, scale = (ring[seed] - outs[seed]).abs(), float(ring[seed].abs().max())
            assert float(d.mean()) <= 1e-2 * scale and float(d.max()) <= 0.3 * scale, (seed, float(d.mean()), float(d.max()), scale)
        model.balanced_tiles = False
        for seed in (1, 2):
            cb = synthetic_batch(hp, 16, seed=seed, t_max=700, force_first_full=True)
            inputs, _, _ = model.parse_batch(dev, cb)
            with torch.no_grad():
                assert torch.equal(ring[seed], model(inputs)[3][0]), seed
    finally:
        ops.USE_SPLITK = True
        model.balanced_tiles = True
