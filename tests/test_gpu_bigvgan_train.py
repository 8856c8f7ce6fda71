"""BigVGAN fine-tuning on the GPU -- K35 (csrc/snake_bwd.hip: the backward of the anti-aliased periodic activation) alone, and whole
generators through `daft_exprt/bigvgan_train.py` -- against tests/bigvgan_grad_oracle.py: float64 autograd through
tests/bigvgan_oracle.py, pinned against plain index sums in tests/test_bigvgan_train_host.py, and never against the code under test.

Tolerances are the two rules of tests/test_gpu_vocoder_train.py (`_bound`), applied per gradient tensor with m = max |o64|:
    fp32   max |g - o64| <= max(8 x max |o32 - o64|, 2e-6 m), o32 the float32 CPU run of the same oracle
    bf16   max |g - o_rounded| <= max(2 d_round, 2e-3 m), d_round = max |o_rounded - o64|
Every test prints its measured values.  NaN stands in every row at or past n[b] of x and dy, and all over dx, dalpha, dinv_beta and
the workspace, before each call of the kernel."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import bigvgan_grad_oracle as BG
from tests import bigvgan_oracle as BO
from tests import vocoder_oracle as O
from tests.test_bigvgan_train_host import INT_DOWN, INT_UP
from tests.test_gpu_vocoder_train import LENGTHS, SEGMENT, T1, T2, TRAIN_CFG, _backward, _bound, _device_mel, _fabricate, _three

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ['fp32', 'bf16']


def _heights():
    from daft_exprt import _hip as H
    out = []
    while H.lib().dx_vocoder_snake_bwd_tile_rows(len(out)) > 0:
        out.append(H.lib().dx_vocoder_snake_bwd_tile_rows(len(out)))
    return out


def _rows(h):
    ''' the two folds at both ends, short of / at / past one tile, and a third tile '''
    return (1, 2, 3, 5, 6, 11, h - 1, h, h + 1, 2 * h + 3)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _taps(f_up, f_down):
    return (ctypes.c_float * 24)(*[float(v) for v in f_up], *[float(v) for v in f_down])


def _kaiser_taps():
    f = BO.kaiser_sinc_filter().float()
    return f, f


def _launch(x, dy, alpha, inv_beta, taps, n, tile_rows=0, N=None, fill=float('nan'), sums=True):
    ''' x, dy (B, C, rows) on the CPU, n the live rows -> (dx (B, N, C), dalpha, dinv_beta) on the device.  `fill` stands in every row
        at or past n[b] of x and dy (up to N), all over dx, the two sums and the workspace '''
    from daft_exprt import _hip as H
    B, c, rows = x.shape
    N = rows if N is None else N

    def rows_major(t):
        out = torch.full((B, N, c), fill, dtype=torch.float32)
        for b, r in enumerate(n):
            out[b, :r] = t[b, :, :r].t().float()
        return out.to(DEV)
    xd, dyd = rows_major(x), rows_major(dy)
    dx = torch.full((B, N, c), fill, dtype=torch.float32, device=DEV)
    da = db = ws = None
    if sums:
        da, db = (torch.full((c,), fill, dtype=torch.float32, device=DEV) for _ in range(2))
        ws = torch.full((H.lib().dx_vocoder_snake_bwd_workspace(B, N, c) // 4,), fill, dtype=torch.float32, device=DEV)
    nd = torch.tensor(n, dtype=torch.int64, device=DEV)
    ad, ibd = alpha.float().to(DEV), inv_beta.float().to(DEV)
    host_taps = _taps(*taps)                                                                 # (kept alive over the call)
    with torch.cuda.device(DEV):
        H.check(H.lib().dx_vocoder_snake_bwd(H.ptr(xd), c, H.ptr(dyd), c, H.ptr(ad), H.ptr(ibd), ctypes.addressof(host_taps), H.ptr(dx), c,
                                             H.ptr(da), H.ptr(db), H.ptr(ws), H.ptr(nd), B, N, c, tile_rows, H.stream()))
        torch.cuda.synchronize()
    return dx, da, db


def _params(c, form, seed):
    ''' (alpha', 1 / (beta' + 1e-9)) fp32 as the kernel receives them: `snake` (beta = alpha) or `snakebeta`, in log scale '''
    g = _gen(seed)
    a, b = 0.5 * torch.randn((c,), generator=g), 0.5 * torch.randn((c,), generator=g)
    return BO.final_params(a, b if form == 'snakebeta' else None, True)


def _case(c, form, h, seed):
    rows = _rows(h)
    B, longest = len(rows), max(rows)
    g = _gen(seed)
    x, dy = torch.randn((B, c, longest), generator=g), torch.randn((B, c, longest), generator=g)
    alpha, inv_beta = _params(c, form, seed + 1)
    taps = _kaiser_taps()
    oracles = _three(lambda dt, rounding: BG.snake_grads(x, dy, alpha, inv_beta, taps, dtype=dt, n=rows))
    return rows, x, dy, alpha, inv_beta, taps, oracles


def _check(got, oracles, rows, what):
    (dx64, da64, db64), (dx32, da32, db32), _ = oracles
    dx, da, db = got
    N = dx.shape[1]
    _bound(dx[:, :dx64.shape[2]].transpose(1, 2), dx64, dx32, None, 'fp32', f'{what}: dx')
    _bound(da, da64, da32, None, 'fp32', f'{what}: dalpha')
    _bound(db, db64, db32, None, 'fp32', f'{what}: dinv_beta')
    for b, r in enumerate(rows):
        assert float(dx[b, r:].abs().max() if r < N else 0.) == 0., (what, b)               # exact zeros, NaN before the call or not


# ---- the kernel alone ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('form', ['snake', 'snakebeta'])
@pytest.mark.parametrize('c', [32, 8, 96])
def test_kernel_against_the_oracle_at_every_tile_height(c, form):
    heights = _heights()
    assert len(heights) >= 2
    for h in heights:
        rows, x, dy, alpha, inv_beta, taps, oracles = _case(c, form, h, seed=c * 10 + h)
        N = max(rows) + h + 5                                                                # more than a tile of dead rows
        _check(_launch(x, dy, alpha, inv_beta, taps, rows, tile_rows=h, N=N), oracles, rows, f'C {c} {form} tile {h}')
    _check(_launch(x, dy, alpha, inv_beta, taps, rows, tile_rows=0, N=N), oracles, rows, f'C {c} {form} tile 0 (the launcher\'s)')


def _integers(B, c, n):
    t, ch, b = torch.arange(n)[None, None, :], torch.arange(c)[None, :, None], torch.arange(B)[:, None, None]
    x = ((3 * t + 5 * ch + b) % 7 - 3).double()
    dy = ((2 * t + 3 * ch + 2 * b) % 5 - 2).double()
    return x, dy


def test_integers_are_exact():
    ''' alpha = inv_beta = 0: du = ds, and with integer taps and small integer x, dy every sum is exact in fp32 -- a tap, row or fold out
        of place changes dx; sin(0) = 0 and 1 - cos(0) = 0 exactly, so both parameter sums are zeros '''
    c, taps = 8, (torch.tensor(INT_UP), torch.tensor(INT_DOWN))
    zeros = torch.zeros((c,))
    for h in _heights():
        rows = _rows(h)
        x, dy = _integers(len(rows), c, max(rows))
        want, _, _ = BG.snake_grads(x, dy, zeros, zeros, taps, n=rows)
        dx, da, db = _launch(x, dy, zeros, zeros, taps, rows, tile_rows=h, N=max(rows) + h + 5)
        assert torch.equal(dx[:, :max(rows)].transpose(1, 2).double().cpu(), want), h
        assert float(da.abs().max()) == 0. and float(db.abs().max()) == 0.


# ---- the contract ------------------------------------------------------------------------------------------------------------

def test_dead_rows_and_the_workspace_are_never_read():
    h = _heights()[0]
    rows, x, dy, alpha, inv_beta, taps, _ = _case(32, 'snakebeta', h, seed=5)
    N = max(rows) + h + 5
    nan = _launch(x, dy, alpha, inv_beta, taps, rows, N=N)
    finite = _launch(x, dy, alpha, inv_beta, taps, rows, N=N, fill=123.5)
    assert all(bool(torch.isfinite(t).all()) for t in nan)
    assert all(torch.equal(a, b) for a, b in zip(nan, finite))
    for b, r in enumerate(rows):
        assert float(nan[0][b, r:].abs().max()) == 0.


def test_an_utterance_gets_the_same_bits_anywhere():
    ''' alone, at another N, beside other neighbours, at every tile height, and without the parameter sums '''
    heights = _heights()
    h = heights[-1]
    rows, x, dy, alpha, inv_beta, taps, (o64, o32, _) = _case(32, 'snakebeta', h, seed=6)
    N = max(rows) + h + 5
    base = _launch(x, dy, alpha, inv_beta, taps, rows, tile_rows=heights[0], N=N)
    again = _launch(x, dy, alpha, inv_beta, taps, rows, tile_rows=heights[0], N=N)
    assert torch.equal(base[1], again[1]) and torch.equal(base[2], again[2]) and torch.equal(base[0], again[0])      # no atomics
    for height in heights[1:] + [0]:
        other = _launch(x, dy, alpha, inv_beta, taps, rows, tile_rows=height, N=N)
        assert torch.equal(other[0], base[0]), height
    without, none_a, none_b = _launch(x, dy, alpha, inv_beta, taps, rows, tile_rows=heights[0], N=N, sums=False)
    assert none_a is None and none_b is None and torch.equal(without, base[0])
    da, db = torch.zeros(32, dtype=torch.float64), torch.zeros(32, dtype=torch.float64)
    for b, r in enumerate(rows):
        alone = _launch(x[b:b + 1, :, :r], dy[b:b + 1, :, :r], alpha, inv_beta, taps, [r])                  # N = r: no dead row at all
        assert torch.equal(alone[0][0], base[0][b, :r]), (b, r)
        da, db = da + alone[1].double().cpu(), db + alone[2].double().cpu()
    order = list(reversed(range(len(rows))))                                                  # other neighbours, another N
    shuffled = _launch(x[order], dy[order], alpha, inv_beta, taps, [rows[i] for i in order], N=N + 17)
    for pos, b in enumerate(order):
        assert torch.equal(shuffled[0][pos, :rows[b]], base[0][b, :rows[b]]), b
    for what, total, got, want64, want32 in (('dalpha', da, base[1], o64[1], o32[1]), ('dinv_beta', db, base[2], o64[2], o32[2])):
        cost, m = float((want32.double() - want64).abs().max()), float(want64.abs().max())
        err, tol = float((got.double().cpu() - total).abs().max()), max(8. * cost, 2e-6 * m)
        print(f'{what}: the batch against the sum of the utterances alone {err:.3g}, bound {tol:.3g}')
        assert err <= tol, (what, err, tol)


def test_conv_post_without_a_gate():
    ''' `_PostUngated`, tanh and clamp, against float64 autograd; the pre-activation has rms 1, so a third of the live samples' gates are shut under the clamp '''
    from daft_exprt import bigvgan_train as BT
    g = _gen(8)
    rows, c = (40, 7, 1), 32
    B, N, n = len(rows), max(rows), torch.tensor(rows)
    x = torch.randn((B, c, N), generator=g)
    w = torch.randn((1, c, 7), generator=g) / (c * 7) ** 0.5
    bias = 0.1 * torch.randn((1,), generator=g)
    proj = torch.randn((B, N), generator=g)
    for clamp in (False, True):
        def oracle(dt, _):
            xs, ws, bs = (t.to(dt).requires_grad_(True) for t in (x, w, bias))
            pre = O.post(O.mask_rows(xs, n), ws, bs, n, slope=1., pre_tanh=True)
            y = O.mask_rows(pre.clamp(-1., 1.) if clamp else torch.tanh(pre), n)
            return (y.detach(),) + torch.autograd.grad((y * proj.to(dt)).sum(), (xs, ws, bs))
        (y64, dx64, dw64, db64), (y32, dx32, dw32, db32), _ = _three(oracle)
        xd = x.transpose(1, 2).contiguous()
        for b, r in enumerate(rows):
            xd[b, r:] = float('nan')
        xd, wd, bd = xd.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
        y = BT._PostUngated.apply(xd, wd, bd, n.to(DEV), clamp)
        dx, dw, db = torch.autograd.grad((y * proj.to(DEV)).sum(), (xd, wd, bd))
        what = 'clamp' if clamp else 'tanh'
        _bound(y, y64, y32, None, 'fp32', f'conv_post {what}: y')
        _bound(dx.transpose(1, 2), O.mask_rows(dx64, n), O.mask_rows(dx32, n), None, 'fp32', f'conv_post {what}: dx')
        _bound(dw, dw64, dw32, None, 'fp32', f'conv_post {what}: dW')
        _bound(db, db64, db32, None, 'fp32', f'conv_post {what}: db')
        if clamp:
            assert 0.05 < float((y64.abs() >= 1.).double().mean()) < 0.5                      # (dead rows count as open)


# ---- whole generators ------------------------------------------------------------------------------------------------------------

CONFIGS = {'T1-snakebeta-log': dict(T1, activation='snakebeta', snake_logscale=True),
           'T2-snake': dict(T2, activation='snake', snake_logscale=False),
           'T1-clamp-no-bias': dict(T1, activation='snakebeta', snake_logscale=True, use_tanh_at_final=False, use_bias_at_final=False)}


@functools.lru_cache(maxsize=None)
def _whole(name):
    ''' (cfg, mel, the state dict the model is built from, projection, the three oracles), computed once.  The model's transposed convs
        are keyed `ups.I.0.*` (upstream's form) in the first config; the oracle's are `ups.I.*`, the parameters' own names '''
    cfg = CONFIGS[name]
    mel = O.make_mel(cfg, LENGTHS, seed=5)
    weights, raw, _, filters = BO.make_weights(cfg, mel, LENGTHS, seed=5)
    sd = BO.state_dict(cfg, weights, raw, None, form='weight_norm', nested_ups=False, seed=5)
    model_sd = BO.state_dict(cfg, weights, raw, filters, form='weight_norm', nested_ups=name == 'T1-snakebeta-log', seed=5)
    proj = torch.randn((len(LENGTHS), max(LENGTHS) * cfg['hop_size']), generator=_gen(6))
    n = torch.tensor(LENGTHS)
    oracles = _three(lambda dt, rounding: BG.generator_grads(cfg, sd, mel, n, proj, rounding=rounding, dtype=dt))
    return cfg, mel, model_sd, proj, oracles


@functools.lru_cache(maxsize=None)
def _generator(name, dtype):
    from daft_exprt.vocoder_train import trainable_generator
    cfg, _, sd, _, _ = _whole(name)
    return trainable_generator(cfg, sd, compute_dtype=dtype).to(DEV)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(CONFIGS))
def test_generator_gradients_match_the_oracle(name, dtype):
    ''' the waveform, the gradient of EVERY parameter -- weight_g, weight_v, bias of every layer, the raw alpha and beta of every
        activation -- and of the mel '''
    from daft_exprt.bigvgan_train import TrainableBigVGAN
    cfg, mel, sd, proj, ((w64, g64, m64), (w32, g32, m32), (wr, gr, mr)) = _whole(name)
    gen = _generator(name, dtype)
    assert type(gen) is TrainableBigVGAN
    wav, grads, dmel = _backward(gen, mel, LENGTHS, proj)
    _bound(wav, w64, w32, wr, dtype, f'{name} waveform')
    assert sorted(grads) == sorted(g64)
    assert any(k.endswith('act.alpha') for k in grads) and any(k.endswith('act.beta') for k in grads) == (cfg['activation'] == 'snakebeta')
    assert ('conv_post.bias' in grads) == cfg.get('use_bias_at_final', True)
    missed = []
    for key in g64:
        assert grads[key].shape == g64[key].shape, key
        try:
            _bound(grads[key], g64[key], g32[key], gr[key], dtype, f'{name} d {key}')
        except AssertionError as e:                                         # every tensor is measured before the test fails
            missed.append(e.args[0])
    _bound(dmel, m64, m32, mr, dtype, f'{name} d mel')
    assert not missed, missed
    for b, t in enumerate(LENGTHS):
        assert float(dmel[b, :, t:].abs().max() if t < max(LENGTHS) else 0.) == 0.


@pytest.mark.parametrize('name', list(CONFIGS))
def test_forward_is_the_inference_paths(name):
    ''' fp32: the same launches on the same weights (T1 and T2 have two ResBlocks per stage: the mean is exact either way) '''
    from daft_exprt.vocoder import Vocoder
    cfg, mel, _, _, _ = _whole(name)
    gen = _generator(name, 'fp32')
    n = torch.tensor(LENGTHS, device=DEV)
    with torch.no_grad():
        wav = gen(mel.to(DEV), n)
    ref, n_samples = Vocoder(cfg, gen.state_dict(), compute_dtype='fp32', device=DEV)(mel.to(DEV), n)
    assert n_samples.tolist() == [t * cfg['hop_size'] for t in LENGTHS]
    print(f'{name}: TrainableBigVGAN against Vocoder {float((wav - ref).abs().max()):.3g}')
    assert torch.equal(wav, ref)


# ---- training ----------------------------------------------------------------------------------------------------------------

BIG_TRAIN_CFG = dict(TRAIN_CFG, activation='snakebeta', snake_logscale=True)


def _pretrained():
    mel = O.make_mel(BIG_TRAIN_CFG, (8,), seed=21)
    weights, raw, _, filters = BO.make_weights(BIG_TRAIN_CFG, mel, (8,), seed=21)
    return BO.state_dict(BIG_TRAIN_CFG, weights, raw, filters, form='weight_norm', nested_ups=True, seed=21)


def test_one_train_step_moves_every_activation_parameter():
    from daft_exprt import vocoder_train as VT
    torch.manual_seed(0)
    gen = VT.trainable_generator(BIG_TRAIN_CFG, _pretrained()).to(DEV)
    mpd, msd = VT.MultiPeriodDiscriminator().to(DEV), VT.MultiScaleDiscriminator().to(DEV)
    optim_g = torch.optim.AdamW(gen.parameters(), VT.LEARNING_RATE, betas=VT.ADAM_BETAS)
    optim_d = torch.optim.AdamW(list(msd.parameters()) + list(mpd.parameters()), VT.LEARNING_RATE, betas=VT.ADAM_BETAS)
    g = _gen(3)
    mel = (torch.randn((2, 80, 8), generator=g) * 1.5 - 4.).to(DEV)
    audio = (0.1 * torch.randn((2, SEGMENT), generator=g)).to(DEV)
    before = {k: p.detach().clone() for k, p in gen.named_parameters() if '.act.' in k}
    assert len(before) == 2 * len(BO.fed_convs(BIG_TRAIN_CFG))
    losses = VT.train_step(gen, mpd, msd, optim_g, optim_d, VT.LossMel(BIG_TRAIN_CFG).to(DEV), mel, audio)
    values = {k: float(v) for k, v in losses.items()}
    print(values)
    assert all(torch.isfinite(torch.tensor(v)) for v in values.values())
    after = dict(gen.named_parameters())
    for k, old in before.items():
        assert bool(torch.isfinite(after[k]).all()) and not bool((after[k] == old).any()), k


def test_train_vocoder_cli_takes_a_bigvgan_checkpoint(tmp_path):
    from daft_exprt.vocoder import Vocoder
    root = _fabricate(str(tmp_path / 'fine_tuning_dataset'), _device_mel)
    pre = tmp_path / 'pretrained'
    pre.mkdir()
    g_path, cfg_path, out = str(pre / 'g_00000000'), str(pre / 'config.json'), str(tmp_path / 'voc')
    torch.save({'generator': _pretrained()}, g_path)
    (pre / 'config.json').write_text(json.dumps(BIG_TRAIN_CFG))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'train_vocoder.py'), '-ft', root, '-cfg', cfg_path, '-g', g_path,
                        '-o', out, '--steps', '3', '--batch_size', '2', '--segment_size', str(SEGMENT), '--checkpoint_interval', '3'],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert sorted(os.listdir(out)) == ['config.json', 'do_00000003', 'g_00000003', 'vocoder_report.json']
    report = json.load(open(os.path.join(out, 'vocoder_report.json')))
    assert report['generator_family'] == 'bigvgan' and report['steps'] == 3
    assert json.load(open(os.path.join(out, 'config.json')))['activation'] == 'snakebeta'
    written = torch.load(os.path.join(out, 'g_00000003'), weights_only=False)['generator']
    assert sorted(written) == sorted(_pretrained())                                          # the source's keys, `ups.I.0.*` and filters
    new = Vocoder.from_checkpoint(os.path.join(out, 'g_00000003'), compute_dtype='fp32', device=DEV)
    old = Vocoder.from_checkpoint(g_path, compute_dtype='fp32', device=DEV)
    mel = (torch.randn((1, 80, 8), generator=_gen(4)) * 1.5 - 4.).to(DEV)
    n = torch.tensor([8], device=DEV)
    wav_new, wav_old = new(mel, n)[0], old(mel, n)[0]
    assert bool(torch.isfinite(wav_new).all()) and float(wav_new.abs().max()) > 0.
    assert float((wav_new - wav_old).abs().max()) > 0.
