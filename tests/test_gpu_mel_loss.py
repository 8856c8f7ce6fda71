"""K37 on the GPU -- one scale of the multi-scale mel loss with its gradient (csrc/mel_loss.hip, `daft_exprt/mel_loss.py`) alone,
`MultiScaleMelLoss` over it, one train step and the script -- against tests/mel_loss_oracle.py: float64 autograd through an explicit
DFT, pinned against `torch.stft` in tests/test_mel_loss_host.py, and never against the code under test.

The tolerance is the project's fp32 rule, per tensor with m = max |o64|:
    max |g - o64| <= max(8 x max |o32 - o64|, 2e-6 m),   o32 the float32 CPU run of the same oracle
computed at run time from the oracle alone; every test prints its measured values.  The gradient is compared with the float64 oracle
differentiated under the kernel's OWN signs sign(Tg - L), taken from the L the kernel wrote (as the dropout tests run the oracle under
the kernel's own masks); an element whose sign differs from the float64 sign must have |Tg - L64| within the case's bound on L.
The cases, their lengths and their seeds are `mel_loss_oracle.CASES` / `SEEDS`.  NaN stands past every n_samples[b] of the waveforms,
in the target's frames past each utterance's, and all over the outputs and the workspace before each call of the kernel."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import mel_loss_oracle as MO
from tests.test_gpu_vocoder_train import SEGMENT, _bound, _device_mel, _fabricate

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(MO.CASES)
NAN = float('nan')


def _tol(o64, o32):
    return max(8. * float((o32.double() - o64).abs().max()), 2e-6 * float(o64.abs().max()))


def _at_clamp(t):
    ''' log10 of the fp32 eps: -5 to two units in the last place of fp32 '''
    return float((t.double() + 5.).abs().max()) <= 1e-6


def _frames(scale, n):
    return [MO.frames_of(k, scale.n_fft, scale.hop, scale.pad) for k in n]


@functools.lru_cache(maxsize=None)
def _case(name):
    ''' (scale, n, audio, wav_hat, the target the kernel is given: the float64 oracle's log-mel of audio rounded to fp32) '''
    scale, n, audio, wav_hat = MO.case_inputs(name)
    return scale, n, audio, wav_hat, MO.log_mel(audio, n, scale).float().double()


@functools.lru_cache(maxsize=None)
def _forward_oracles(name):
    ''' per dtype (L of audio, L of wav_hat, loss), computed once and left unchanged '''
    scale, n, audio, wav_hat, target = _case(name)
    out = []
    for dt in (torch.float64, torch.float32):
        own, loss, _ = MO.loss_and_gradient(wav_hat, target, n, scale, dt)
        out.append((MO.log_mel(audio, n, scale, dt), own, loss))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _tables(scale_key):
    ''' device tables of a scale: (twiddle, window, fb, fb_lo, fb_hi, bin_lo, bin_hi) '''
    from daft_exprt import _hip as H
    from daft_exprt.mel_loss import band_tables
    scale = _SCALES[scale_key]
    t = torch.empty(2 * scale.n_fft, dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        H.check(H.lib().dx_mel_loss_tables(H.ptr(t), scale.n_fft, H.stream()))
    bands = band_tables(scale.fb.float().numpy())
    return (t, scale.window.float().to(DEV), scale.fb.float().contiguous().to(DEV)) + tuple(torch.from_numpy(b).to(DEV) for b in bands)


_SCALES = {}


def _key(scale):
    key = (scale.n_fft, scale.hop, scale.pad, tuple(scale.fb.shape), float(scale.fb.sum()))
    _SCALES.setdefault(key, scale)
    return key


def _launch(scale, n, audio, wav_hat, target, fill=NAN, S=None, T=None, factor=1., own=True):
    ''' CPU tensors -> (L of audio (B, T, M) by the log-mel entry point, L of wav_hat (or None), loss (B,), dwav (B, S)) on the device.
        `fill` stands past n[b] of both waveforms, in the target's frames past each utterance's, and all over the outputs and the workspace '''
    from daft_exprt import _hip as H
    B, M, frames = len(n), scale.fb.shape[0], _frames(scale, n)
    S, T = max(n) if S is None else S, max(frames) if T is None else T
    ad, wd = torch.full((B, S), fill, dtype=torch.float32), torch.full((B, S), fill, dtype=torch.float32)
    td = torch.full((B, T, M), fill, dtype=torch.float32)
    for b, (k, f) in enumerate(zip(n, frames)):
        ad[b, :k], wd[b, :k], td[b, :f] = audio[b, :k].float(), wav_hat[b, :k].float(), target[b, :f].float()
    ad, wd, td = ad.to(DEV), wd.to(DEV), td.to(DEV)
    la, lw = (torch.full((B, T, M), fill, dtype=torch.float32, device=DEV) for _ in range(2))
    loss = torch.full((B,), fill, dtype=torch.float32, device=DEV)
    dwav = torch.full((B, S), fill, dtype=torch.float32, device=DEV)
    lib = H.lib()
    ws = torch.full((lib.dx_mel_loss_workspace(B, T, M, scale.n_fft) // 4,), fill, dtype=torch.float32, device=DEV)
    nd, nh = torch.tensor(n, dtype=torch.int64, device=DEV), (ctypes.c_int64 * B)(*n)
    tw, win, fb, fb_lo, fb_hi, bin_lo, bin_hi = _tables(_key(scale))
    with torch.cuda.device(DEV):
        H.check(lib.dx_mel_loss_log_mel(H.ptr(ad), S, H.ptr(nd), ctypes.addressof(nh), H.ptr(tw), H.ptr(win), H.ptr(fb), H.ptr(fb_lo),
                                        H.ptr(fb_hi), H.ptr(la), B, S, T, M, scale.n_fft, scale.hop, scale.pad, scale.eps, H.stream()))
        H.check(lib.dx_mel_loss(H.ptr(wd), S, H.ptr(nd), ctypes.addressof(nh), H.ptr(tw), H.ptr(win), H.ptr(fb), H.ptr(fb_lo), H.ptr(fb_hi),
                                H.ptr(bin_lo), H.ptr(bin_hi), H.ptr(td), factor, H.ptr(loss), H.ptr(dwav), S, H.ptr(lw) if own else None,
                                H.ptr(ws), B, S, T, M, scale.n_fft, scale.hop, scale.pad, scale.eps, H.stream()))
        torch.cuda.synchronize()
    return la, (lw if own else None), loss, dwav


# ---- the kernel alone ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
def test_kernel_against_the_oracle(name):
    scale, n, audio, wav_hat, target = _case(name)
    (la64, own64, loss64), (la32, own32, loss32) = _forward_oracles(name)
    frames, T = _frames(scale, n), own64.shape[1]
    la, own, loss, dwav = _launch(scale, n, audio, wav_hat, target, S=max(n) + 17, T=T + 3)
    missed = []

    def bound(*args):
        try:
            _bound(*args)
        except AssertionError as e:                                          # every tensor is measured before the test fails
            missed.append(e.args[0])
    bound(la[:, :T], la64, la32, None, 'fp32', f'{name} n {n}: L of the target')
    bound(own[:, :T], own64, own32, None, 'fp32', f'{name} n {n}: L')
    bound(loss, loss64, loss32, None, 'fp32', f'{name} n {n}: loss')
    # the gradient under the kernel's own signs
    tol_l = _tol(own64, own32)
    signs = torch.sign(target.float() - own[:, :T].cpu()).double()
    signs64 = torch.sign(target - own64)
    differ = torch.zeros_like(signs, dtype=torch.bool)
    for b, f in enumerate(frames):
        differ[b, :f] = signs[b, :f] != signs64[b, :f]
    worst = float((target - own64).abs()[differ].max()) if bool(differ.any()) else 0.
    print(f'{name}: {int(differ.sum())} of {sum(frames) * own64.shape[2]} signs differ from float64, the largest |Tg - L64| there {worst:.3g} '
          f'(bound on L {tol_l:.3g})')
    assert worst <= tol_l, (name, worst, tol_l)
    (_, _, dwav64), (_, _, dwav32) = (MO.loss_and_gradient(wav_hat, target, n, scale, dt, signs=signs) for dt in (torch.float64, torch.float32))
    bound(dwav[:, :max(n)], dwav64, dwav32, None, 'fp32', f'{name} n {n}: dwav')
    assert not missed, missed
    for b, (k, f) in enumerate(zip(n, frames)):                              # exact zeros over NaN
        assert float(la[b, f:].abs().max()) == 0. and float(own[b, f:].abs().max()) == 0. and float(dwav[b, k:].abs().max()) == 0., (name, b)


def test_empty_filters_sit_at_the_clamp_and_carry_no_gradient():
    scale, n, audio, wav_hat, target = _case('256-empty')
    empty = (scale.fb.sum(1) == 0)
    assert int(empty.sum()) > 100
    la, own, loss, dwav = _launch(scale, n, audio, wav_hat, target)
    for b, f in enumerate(_frames(scale, n)):
        assert _at_clamp(la[b, :f][:, empty.to(DEV)]) and _at_clamp(own[b, :f][:, empty.to(DEV)])
    full = MO.make_scale(256, 320)
    live = MO.Scale(full.n_fft, full.hop, full.pad, full.window, full.fb[~empty], full.eps)
    _, _, loss2, dwav2 = _launch(live, n, audio, wav_hat, target[:, :, ~empty])
    assert torch.equal(dwav, dwav2)                                         # the empty rows add nothing to any bin's sum


def test_the_scale_factor_multiplies_the_gradient_only():
    scale, n, audio, wav_hat, target = _case('64-10')
    _, _, loss, dwav = _launch(scale, n, audio, wav_hat, target)
    _, _, loss4, dwav4 = _launch(scale, n, audio, wav_hat, target, factor=0.25, own=False)
    assert torch.equal(loss, loss4) and torch.equal(dwav4, dwav * 0.25)


# ---- the contract ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['32-10', '128-20', '256-general', '2048-320'])
def test_nothing_dead_is_read(name):
    scale, n, audio, wav_hat, target = _case(name)
    S, T = max(n) + 9, max(_frames(scale, n)) + 2
    nan = _launch(scale, n, audio, wav_hat, target, S=S, T=T)
    finite = _launch(scale, n, audio, wav_hat, target, fill=123.5, S=S, T=T)
    assert all(bool(torch.isfinite(t).all()) for t in nan)
    assert all(torch.equal(a, b) for a, b in zip(nan, finite))


@pytest.mark.parametrize('name', ['32-5', '64-10', '256-40', '512-80', '1024-160'])
def test_an_utterance_gets_the_same_bits_anywhere(name):
    ''' a second call, alone, beside other neighbours, at a larger T and a wider row '''
    scale, n, audio, wav_hat, target = _case(name)
    base = _launch(scale, n, audio, wav_hat, target)
    again = _launch(scale, n, audio, wav_hat, target)
    assert all(torch.equal(a, b) for a, b in zip(base, again))                              # no atomics
    frames = _frames(scale, n)
    for b, (k, f) in enumerate(zip(n, frames)):
        alone = _launch(scale, [k], audio[b:b + 1], wav_hat[b:b + 1], target[b:b + 1])          # S = n, T = F: nothing dead at all
        assert torch.equal(alone[0][0], base[0][b, :f]) and torch.equal(alone[1][0], base[1][b, :f]), (name, b)
        assert torch.equal(alone[2][0], base[2][b]) and torch.equal(alone[3][0], base[3][b, :k]), (name, b)
    order = [2, 0, 1]
    shuffled = _launch(scale, [n[i] for i in order], audio[order], wav_hat[order], target[order], S=max(n) + 33, T=max(frames) + 5)
    for pos, b in enumerate(order):
        assert torch.equal(shuffled[0][pos, :frames[b]], base[0][b, :frames[b]]) and torch.equal(shuffled[1][pos, :frames[b]], base[1][b, :frames[b]])
        assert torch.equal(shuffled[2][pos], base[2][b]) and torch.equal(shuffled[3][pos, :n[b]], base[3][b, :n[b]]), (name, b)


@pytest.mark.parametrize('n_fft,n_mels', list(zip(MO.WINDOW_LENGTHS, MO.N_MELS)))
def test_silence_is_exact(n_fft, n_mels):
    ''' an all-zero pair, the target from the log-mel entry point: both log-mels sit at the clamp with the same bits, loss = 0 and
        dwav = 0 exactly (never NaN), beside a live neighbour '''
    scale = MO.make_scale(n_fft, n_mels)
    n = [2 * n_fft + 3, 2 * n_fft - 7]
    g = torch.Generator().manual_seed(n_fft)
    audio, wav_hat = torch.zeros((2, max(n)), dtype=torch.float64), torch.zeros((2, max(n)), dtype=torch.float64)
    audio[1] = (0.3 * torch.randn((max(n),), generator=g, dtype=torch.float64)).float().double()
    wav_hat[1] = (audio[1] + 0.15 * torch.randn((max(n),), generator=g, dtype=torch.float64)).float().double()
    la, _, _, _ = _launch(scale, n, audio, wav_hat, MO.log_mel(audio, n, scale))
    la, own, loss, dwav = _launch(scale, n, audio, wav_hat, la.cpu().double())       # the target as the log-mel entry point wrote it
    f0 = _frames(scale, n)[0]
    assert torch.equal(la[0, :f0], own[0, :f0])
    assert _at_clamp(la[0, :f0]) and _at_clamp(own[0, :f0])
    assert float(loss[0]) == 0. and float(dwav[0].abs().max()) == 0.
    assert float(loss[1]) > 0. and float(dwav[1].abs().max()) > 0. and bool(torch.isfinite(dwav).all())


def test_a_waveform_below_the_clamp_gets_no_gradient():
    ''' amplitude 1e-7: every mel is below eps, so dwav = 0 exactly and loss = sum |Tg + 5| '''
    scale, n, audio, wav_hat, target = _case('128-20')
    quiet = (1e-7 * wav_hat).float().double()
    _, own, loss, dwav = _launch(scale, n, audio, quiet, target)
    assert float(dwav.abs().max()) == 0.
    own64, loss64, _ = MO.loss_and_gradient(quiet, target, n, scale)
    _, loss32, _ = MO.loss_and_gradient(quiet, target, n, scale, torch.float32)
    for b, f in enumerate(_frames(scale, n)):
        assert _at_clamp(own[b, :f]) and float((own64[b, :f] + 5.).abs().max()) <= 1e-12
        assert abs(float(loss64[b]) - float((target[b, :f] + 5.).abs().sum())) <= 1e-9 * float(loss64[b])
    _bound(loss, loss64, loss32, None, 'fp32', 'below the clamp: loss')


def test_refusals_come_before_any_launch():
    from daft_exprt import _hip as H
    lib = H.lib()
    scale = MO.make_scale(64, 10)
    tw, win, fb, fb_lo, fb_hi, bin_lo, bin_hi = _tables(_key(scale))
    B, S, T, M = 2, 300, 19, 10
    wav = torch.zeros((B, S), dtype=torch.float32, device=DEV)
    out = torch.full((B, T, M), NAN, dtype=torch.float32, device=DEV)
    loss, dwav = torch.full((B,), NAN, dtype=torch.float32, device=DEV), torch.full((B, S), NAN, dtype=torch.float32, device=DEV)
    ws = torch.empty((lib.dx_mel_loss_workspace(B, T, M, 64) // 4,), dtype=torch.float32, device=DEV)
    nd = torch.tensor([300, 32], dtype=torch.int64, device=DEV)

    def call(n=(300, 32), n_fft=64, hop=16, pad=32, m=M, eps=1e-5):
        nh = (ctypes.c_int64 * B)(*n)
        a = lib.dx_mel_loss_log_mel(H.ptr(wav), S, H.ptr(nd), ctypes.addressof(nh), H.ptr(tw), H.ptr(win), H.ptr(fb), H.ptr(fb_lo), H.ptr(fb_hi),
                                    H.ptr(out), B, S, T, m, n_fft, hop, pad, eps, H.stream())
        msg = lib.dx_last_error()
        b = lib.dx_mel_loss(H.ptr(wav), S, H.ptr(nd), ctypes.addressof(nh), H.ptr(tw), H.ptr(win), H.ptr(fb), H.ptr(fb_lo), H.ptr(fb_hi),
                            H.ptr(bin_lo), H.ptr(bin_hi), H.ptr(out), 1., H.ptr(loss), H.ptr(dwav), S, None, H.ptr(ws), B, S, T, m, n_fft, hop,
                            pad, eps, H.stream())
        return a, b, msg + b' | ' + lib.dx_last_error()
    with torch.cuda.device(DEV):
        for kwargs, word in ((dict(), b'utterance 1 has 32 samples'), (dict(n=(300, 40), pad=0), b'utterance 1 has 40 samples'),
                             (dict(n_fft=96), b'n_fft=96'), (dict(hop=65), b'hop=65'), (dict(hop=0), b'hop=0'), (dict(m=0), b'M=0'),
                             (dict(eps=0.), b'eps')):
            a, b, msg = call(**kwargs)
            assert a == b == -5 and msg.count(word) == 2, (kwargs, a, b, msg)
        torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(loss).all()) and bool(torch.isnan(dwav).all())      # nothing was launched


# ---- the differentiable op and the module ------------------------------------------------------------------------------------

def test_autograd_function_is_the_launch():
    ''' `log_mel` / `log_mel_l1`: the launches' bits, n_samples as a device tensor or a host list, a strided waveform, the factor '''
    from daft_exprt.mel_loss import MelScale, log_mel, log_mel_l1
    scale, n, audio, wav_hat, _ = _case('64-10')
    s = MelScale(scale.n_fft, scale.hop, scale.pad, scale.window.float(), scale.fb.float(), scale.eps)
    ad, wd = torch.full(audio.shape, NAN, dtype=torch.float32), torch.full(audio.shape, NAN, dtype=torch.float32)
    for b, k in enumerate(n):
        ad[b, :k], wd[b, :k] = audio[b, :k].float(), wav_hat[b, :k].float()
    for counts in (torch.tensor(n, dtype=torch.int64, device=DEV), list(n)):
        target = log_mel(ad.to(DEV), counts, s)
        la, _, loss, dwav = _launch(scale, n, audio, wav_hat, target.cpu().double(), fill=0.)
        assert torch.equal(target, la)
        wide = torch.full((len(n), max(n) + 5), NAN, dtype=torch.float32, device=DEV)
        wide[:, :max(n)] = wd.to(DEV)
        x = wide.requires_grad_(True)
        value = log_mel_l1(x[:, :max(n)], target, counts, s, factor=0.5)
        (3. * value).backward()
        assert torch.equal(value.detach(), loss.sum() * 0.5)
        assert torch.equal(x.grad[:, :max(n)], dwav * 0.5 * 3.) and float(x.grad[:, max(n):].abs().max()) == 0.
    with pytest.raises(ValueError, match=r'too few.*utterance 1'):
        log_mel(ad.to(DEV), [n[0], 3, n[2]], s)
    with pytest.raises(ValueError, match='target'):
        log_mel_l1(wd.to(DEV), target[:, :3], list(n), s)


def test_module_against_the_oracle():
    ''' the seven default scales, B = 2, segment 2048: the value and the waveform gradient, the float64 oracle under the kernel's signs '''
    from daft_exprt.mel_loss import MultiScaleMelLoss, log_mel, log_mel_l1_launch
    from tests.test_gpu_bigvgan_train import BIG_TRAIN_CFG
    audio, y_hat = MO.module_inputs()
    assert audio.shape == (2, 2048)
    module = MultiScaleMelLoss(BIG_TRAIN_CFG)
    assert module.weight == 15. and len(module.scales) == 7
    a, x = audio.float().to(DEV), y_hat.float().to(DEV).requires_grad_(True)
    value = module(a, x)
    value.backward()
    n, signs = [2048, 2048], []
    for s in module.scales:
        target = log_mel(a, n, s)
        _, _, own = log_mel_l1_launch(x.detach(), target, n, s, want_log_mel=True)
        signs.append(torch.sign(target - own).cpu().double())
    (v64, g64, _), (v32, g32, _) = (MO.module_loss(audio, y_hat, dt, signs) for dt in (torch.float64, torch.float32))
    _bound(value.detach().reshape(1), v64.reshape(1), v32.reshape(1), None, 'fp32', 'MultiScaleMelLoss value')
    _bound(x.grad, g64, g32, None, 'fp32', 'MultiScaleMelLoss d y_hat')


# ---- training ----------------------------------------------------------------------------------------------------------------

def test_one_train_step_with_the_multiscale_mel_loss():
    from daft_exprt import vocoder_train as VT
    from daft_exprt.mel_loss import MultiScaleMelLoss
    from tests.test_gpu_bigvgan_train import BIG_TRAIN_CFG, _pretrained
    torch.manual_seed(0)
    gen = VT.trainable_generator(BIG_TRAIN_CFG, _pretrained()).to(DEV)
    mpd, msd = VT.MultiPeriodDiscriminator().to(DEV), VT.MultiScaleDiscriminator().to(DEV)
    optim_g = torch.optim.AdamW(gen.parameters(), VT.LEARNING_RATE, betas=VT.ADAM_BETAS)
    optim_d = torch.optim.AdamW(list(msd.parameters()) + list(mpd.parameters()), VT.LEARNING_RATE, betas=VT.ADAM_BETAS)
    g = torch.Generator().manual_seed(3)
    mel = (torch.randn((2, 80, 8), generator=g) * 1.5 - 4.).to(DEV)
    audio = (0.1 * torch.randn((2, SEGMENT), generator=g)).to(DEV)
    before = {k: p.detach().clone() for k, p in gen.named_parameters()}
    module = MultiScaleMelLoss(BIG_TRAIN_CFG)
    module.check_segment(SEGMENT)
    losses = VT.train_step(gen, mpd, msd, optim_g, optim_d, VT.LossMel(BIG_TRAIN_CFG).to(DEV), mel, audio, mel_loss=module)
    values = {k: float(v) for k, v in losses.items()}
    print(values)
    assert sorted(values) == ['adv', 'disc', 'fm', 'mel'] and all(torch.isfinite(torch.tensor(v)) for v in values.values())
    for k, p in gen.named_parameters():
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[k]), k


def _script(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'train_vocoder.py'), *args], capture_output=True, text=True, timeout=300)


def test_train_vocoder_cli_with_the_multiscale_mel_loss(tmp_path):
    from tests.test_gpu_bigvgan_train import BIG_TRAIN_CFG, _pretrained
    root = _fabricate(str(tmp_path / 'fine_tuning_dataset'), _device_mel)
    pre = tmp_path / 'pretrained'
    pre.mkdir()
    g_path, cfg_path = str(pre / 'g_00000000'), str(pre / 'config.json')
    torch.save({'generator': _pretrained()}, g_path)
    (pre / 'config.json').write_text(json.dumps(BIG_TRAIN_CFG))
    common = ['-ft', root, '-cfg', cfg_path, '-g', g_path, '--steps', '3', '--batch_size', '2', '--segment_size', str(SEGMENT),
              '--checkpoint_interval', '3']
    for flags, want in ((['--mel_loss', 'multiscale'], 'multiscale'), ([], 'single')):
        out = str(tmp_path / f'voc_{want}')
        r = _script(*common, '-o', out, *flags)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert sorted(os.listdir(out)) == ['config.json', 'do_00000003', 'g_00000003', 'vocoder_report.json']
        report = json.load(open(os.path.join(out, 'vocoder_report.json')))
        assert report['mel_loss'] == want and report['steps'] == 3 and report['second_discriminator'] == 'msd'
        assert all(torch.isfinite(torch.tensor(entry['mel'])) for entry in report['log'])
    r = _script(*common, '-o', str(tmp_path / 'voc_short'), '--mel_loss', 'multiscale', '--segment_size', '1024')
    assert r.returncode != 0 and 'too short for the scale (n_fft 2048' in r.stderr, r.stderr[-2000:]
