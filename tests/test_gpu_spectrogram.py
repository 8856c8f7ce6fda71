"""K36 on the GPU -- the magnitude spectrogram of a waveform and its gradient (csrc/spectrogram.hip, `daft_exprt/spectrogram.py`) alone,
BigVGAN's `DiscriminatorR` over it, one MPD + MRD train step and the script -- against tests/spectrogram_oracle.py: float64 autograd
through an explicit DFT, pinned against `torch.stft` in tests/test_spectrogram_host.py, and never against the code under test.

The tolerance is the fp32 rule of tests/test_gpu_vocoder_train.py (`_bound`), per tensor with m = max |o64|:
    max |g - o64| <= max(8 x max |o32 - o64|, 2e-6 m),   o32 the float32 CPU run of the same oracle
Every test prints its measured values.  The cases, their lengths and their seeds are `spectrogram_oracle.CASES`; the host file asserts
that each is well conditioned (min |X| >= 1e-3 max |X|).  NaN stands past every n_samples[b] of wav, in the frames of dmag past each
utterance's, and all over mag, dwav and the workspace before each call of the kernel."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import spectrogram_oracle as SO
from tests.test_gpu_vocoder_train import SEGMENT, _bound, _device_mel, _fabricate

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in SO.CASES]
NAN = float('nan')


@functools.lru_cache(maxsize=None)
def _oracles(name):
    ''' ((mag64, dwav64), (mag32, dwav32)), computed once and left unchanged '''
    n_fft, hop, window, n, wav, dmag = SO.case_inputs(name)
    return tuple(SO.spectrogram(wav, n, n_fft, hop, window, dtype=dt, dmag=dmag) for dt in (torch.float64, torch.float32))


@functools.lru_cache(maxsize=None)
def _twiddle(n_fft):
    from daft_exprt import _hip as H
    t = torch.empty(2 * n_fft, dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        H.check(H.lib().dx_spectrogram_tables(H.ptr(t), n_fft, H.stream()))
    return t


def _launch(n_fft, hop, window, n, wav, dmag, fill=NAN, S=None, T=None, backward=True):
    ''' wav (B, >= max n), dmag (B, bins, >= max frames) on the CPU -> (mag (B, bins, T), dwav (B, S)) on the device.  `fill` stands past
        n[b] of wav, in the frames of dmag past each utterance's, and all over mag, dwav and the workspace '''
    from daft_exprt import _hip as H
    B, bins = len(n), n_fft // 2 + 1
    frames = [SO.frames_of(k, n_fft, hop) for k in n]
    S, T = max(n) if S is None else S, max(frames) if T is None else T
    wd, gd = torch.full((B, S), fill, dtype=torch.float32), torch.full((B, bins, T), fill, dtype=torch.float32)
    for b, (k, f) in enumerate(zip(n, frames)):
        wd[b, :k] = wav[b, :k].float()
        gd[b, :, :f] = dmag[b, :, :f].float()
    wd, gd, win = wd.to(DEV), gd.to(DEV), window.float().to(DEV)
    mag = torch.full((B, bins, T), fill, dtype=torch.float32, device=DEV)
    dwav = torch.full((B, S), fill, dtype=torch.float32, device=DEV)
    ws = torch.full((H.lib().dx_spectrogram_bwd_workspace(B, T, n_fft) // 4,), fill, dtype=torch.float32, device=DEV)
    nd, nh = torch.tensor(n, dtype=torch.int64, device=DEV), (ctypes.c_int64 * B)(*n)
    with torch.cuda.device(DEV):
        H.check(H.lib().dx_spectrogram(H.ptr(wd), S, H.ptr(nd), ctypes.addressof(nh), H.ptr(_twiddle(n_fft)), H.ptr(win), H.ptr(mag), B, S, T,
                                       n_fft, hop, H.stream()))
        if backward:
            H.check(H.lib().dx_spectrogram_bwd(H.ptr(wd), S, H.ptr(nd), ctypes.addressof(nh), H.ptr(_twiddle(n_fft)), H.ptr(win), H.ptr(gd),
                                               H.ptr(dwav), S, H.ptr(ws), B, S, T, n_fft, hop, H.stream()))
        torch.cuda.synchronize()
    return mag, dwav


# ---- the kernel alone ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
def test_kernel_against_the_oracle(name):
    n_fft, hop, window, n, wav, dmag = SO.case_inputs(name)
    (mag64, dwav64), (mag32, dwav32) = _oracles(name)
    mag, dwav = _launch(n_fft, hop, window, n, wav, dmag, S=max(n) + 17, T=mag64.shape[2] + 3)
    _bound(mag[:, :, :mag64.shape[2]], mag64, mag32, None, 'fp32', f'{name} n {n}: mag')
    _bound(dwav[:, :max(n)], dwav64, dwav32, None, 'fp32', f'{name} n {n}: dwav')
    for b, k in enumerate(n):
        f = SO.frames_of(k, n_fft, hop)
        assert float(mag[b, :, f:].abs().max()) == 0. and float(dwav[b, k:].abs().max()) == 0., (name, b)     # exact zeros over NaN


def test_frame_counts_at_the_shortest_lengths():
    ''' n = p + 1, where the two reflected stretches overlap: F = 4 / 3 / 3 '''
    got = {c[1]: SO.frames_of(c[4][0], c[1], c[2]) for c in SO.CASES if c[0].endswith('-a')}
    assert got == {512: 4, 1024: 3, 2048: 3}


# ---- the contract ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['512-50-240-b', '2048-240-1200-a', '256-64-hann'])
def test_nothing_dead_is_read(name):
    args = SO.case_inputs(name)
    n, frames = args[3], [SO.frames_of(k, args[0], args[1]) for k in args[3]]
    S, T = max(n) + 9, max(frames) + 2
    nan = _launch(*args, S=S, T=T)
    finite = _launch(*args, fill=123.5, S=S, T=T)
    assert all(bool(torch.isfinite(t).all()) for t in nan)
    assert all(torch.equal(a, b) for a, b in zip(nan, finite))


@pytest.mark.parametrize('name', ['512-50-240-a', '1024-120-600-b', '2048-240-1200-b', '4096-1024-hann'])
def test_an_utterance_gets_the_same_bits_anywhere(name):
    ''' a second call, alone, beside other neighbours, at a larger T and a wider row '''
    n_fft, hop, window, n, wav, dmag = SO.case_inputs(name)
    base = _launch(n_fft, hop, window, n, wav, dmag)
    again = _launch(n_fft, hop, window, n, wav, dmag)
    assert torch.equal(base[0], again[0]) and torch.equal(base[1], again[1])                # no atomics
    frames = [SO.frames_of(k, n_fft, hop) for k in n]
    for b, (k, f) in enumerate(zip(n, frames)):
        alone = _launch(n_fft, hop, window, [k], wav[b:b + 1], dmag[b:b + 1])                # S = n, T = F: nothing dead at all
        assert torch.equal(alone[0][0], base[0][b, :, :f]) and torch.equal(alone[1][0], base[1][b, :k]), (name, b)
    order = [2, 0, 1]
    shuffled = _launch(n_fft, hop, window, [n[i] for i in order], wav[order], dmag[order], S=max(n) + 33, T=max(frames) + 5)
    for pos, b in enumerate(order):
        assert torch.equal(shuffled[0][pos, :, :frames[b]], base[0][b, :, :frames[b]]), (name, b)
        assert torch.equal(shuffled[1][pos, :n[b]], base[1][b, :n[b]]), (name, b)


@pytest.mark.parametrize('n_fft,hop,win', SO.RESOLUTIONS + ((256, 64, 256), (4096, 1024, 4096)))
def test_silence_is_exact(n_fft, hop, win):
    ''' |X| = 0 everywhere: mag = 0 and, the norm's gradient being 0 there (never NaN), dwav = 0, beside a live neighbour '''
    p = (n_fft - hop) // 2
    n = [2 * p + n_fft, 2 * p + n_fft - 7]
    g = torch.Generator().manual_seed(n_fft)
    wav = torch.zeros((2, max(n)), dtype=torch.float64)
    wav[1] = torch.randn((max(n),), generator=g, dtype=torch.float64)
    T = max(SO.frames_of(k, n_fft, hop) for k in n)
    dmag = torch.randn((2, n_fft // 2 + 1, T), generator=g, dtype=torch.float64)
    mag, dwav = _launch(n_fft, hop, SO.window_table(n_fft, win), n, wav, dmag)
    assert float(mag[0].abs().max()) == 0. and float(dwav[0].abs().max()) == 0.
    assert float(mag[1].abs().max()) > 0. and float(dwav[1].abs().max()) > 0. and bool(torch.isfinite(dwav).all())


# ---- the differentiable op ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['1024-120-600-a', '256-64-hann'])
def test_autograd_function_is_the_two_launches(name):
    ''' `spectrogram()`: the launches' bits, frames on the device, a non-contiguous dmag, n_samples as a device tensor or a host list '''
    from daft_exprt.spectrogram import spectrogram
    n_fft, hop, window, n, wav, dmag = SO.case_inputs(name)
    _, _, win, _ = next(c for c in SO.CASES if c[0] == name)[1:]
    base_mag, base_dwav = _launch(n_fft, hop, window, n, wav, dmag, fill=0.)
    wd = torch.zeros((len(n), max(n)), dtype=torch.float32)
    for b, k in enumerate(n):
        wd[b, :k] = wav[b, :k].float()
        wd[b, k:] = NAN
    frames = [SO.frames_of(k, n_fft, hop) for k in n]
    gd = dmag.float()
    for b, f in enumerate(frames):
        gd[b, :, f:] = NAN
    strided = gd.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
    assert not strided.is_contiguous()
    for counts in (torch.tensor(n, dtype=torch.int64, device=DEV), list(n)):
        x = wd.to(DEV).requires_grad_(True)
        kwargs = dict(window=window.float()) if win == 'hann' else dict(win=win)
        mag, got_frames = spectrogram(x, counts, n_fft, hop, **kwargs)
        assert got_frames.tolist() == frames and got_frames.device.type == 'cuda'
        mag.backward(strided)
        assert torch.equal(mag.detach(), base_mag) and torch.equal(x.grad, base_dwav)
    with pytest.raises(ValueError, match=r'too few.*utterance 1'):
        spectrogram(wd.to(DEV), [n[0], 3, n[2]], n_fft, hop)


# ---- the module --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('resolution', SO.RESOLUTIONS)
def test_discriminator_r_against_the_oracle_module(resolution):
    ''' scores, every feature map and the waveform gradient of sum(score), the float64 oracle module on the same weights and signals '''
    from daft_exprt import bigvgan_train as BT
    sd = {k: v.float().double() for k, v in SO.make_r_weights(seed=resolution[0]).items()}
    wav = SO.module_wav(resolution)
    assert wav.shape == (2, 2048)
    (s64, f64, g64), (s32, f32, g32) = (SO.discriminator_r(sd, wav, resolution, dtype=dt, proj=True) for dt in (torch.float64, torch.float32))
    d = BT.DiscriminatorR(resolution).to(DEV)
    d.load_state_dict({k: v.float() for k, v in sd.items()})
    x = wav.float().to(DEV)[:, None].requires_grad_(True)
    scores, fmap = d(x)
    scores.sum().backward()
    missed = []
    for what, got, o64, o32 in [('scores', scores, s64, s32)] + [(f'fmap {i}', a, b, c) for i, (a, b, c) in enumerate(zip(fmap, f64, f32))] + \
            [('d wav', x.grad[:, 0], g64, g32)]:
        try:
            _bound(got, o64, o32, None, 'fp32', f'DiscriminatorR {resolution} {what}')
        except AssertionError as e:                                         # every tensor is measured before the test fails
            missed.append(e.args[0])
    assert len(fmap) == 6 and not missed, missed


# ---- training ----------------------------------------------------------------------------------------------------------------

def test_one_train_step_with_mpd_and_mrd():
    from daft_exprt import bigvgan_train as BT
    from daft_exprt import vocoder_train as VT
    from tests.test_gpu_bigvgan_train import BIG_TRAIN_CFG, _pretrained
    torch.manual_seed(0)
    gen = VT.trainable_generator(BIG_TRAIN_CFG, _pretrained()).to(DEV)
    mpd, mrd = VT.MultiPeriodDiscriminator().to(DEV), BT.MultiResolutionDiscriminator(BIG_TRAIN_CFG).to(DEV)
    optim_g = torch.optim.AdamW(gen.parameters(), VT.MRD_LEARNING_RATE, betas=VT.ADAM_BETAS)
    optim_d = torch.optim.AdamW(list(mrd.parameters()) + list(mpd.parameters()), VT.MRD_LEARNING_RATE, betas=VT.ADAM_BETAS)
    g = torch.Generator().manual_seed(3)
    mel = (torch.randn((2, 80, 8), generator=g) * 1.5 - 4.).to(DEV)
    audio = (0.1 * torch.randn((2, SEGMENT), generator=g)).to(DEV)
    before_d = {k: p.detach().clone() for k, p in mrd.named_parameters()}
    before_g = {k: p.detach().clone() for k, p in gen.named_parameters()}
    assert len(before_d) == 3 * 6 * 3
    losses = VT.train_step(gen, mpd, mrd, optim_g, optim_d, VT.LossMel(BIG_TRAIN_CFG).to(DEV), mel, audio,
                           clip_grad_norm=VT.MRD_CLIP_GRAD_NORM)
    values = {k: float(v) for k, v in losses.items()}
    print(values)
    assert sorted(values) == ['adv', 'disc', 'fm', 'mel'] and all(torch.isfinite(torch.tensor(v)) for v in values.values())
    for before, module in ((before_d, mrd), (before_g, gen)):
        for k, p in module.named_parameters():
            assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[k]), k


def _script(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'train_vocoder.py'), *args], capture_output=True, text=True, timeout=300)


def test_train_vocoder_cli_with_mrd(tmp_path):
    from tests.test_gpu_bigvgan_train import BIG_TRAIN_CFG, _pretrained
    root = _fabricate(str(tmp_path / 'fine_tuning_dataset'), _device_mel)
    pre = tmp_path / 'pretrained'
    pre.mkdir()
    g_path, cfg_path, out = str(pre / 'g_00000000'), str(pre / 'config.json'), str(tmp_path / 'voc')
    torch.save({'generator': _pretrained()}, g_path)
    (pre / 'config.json').write_text(json.dumps(BIG_TRAIN_CFG))
    common = ['-ft', root, '-cfg', cfg_path, '-g', g_path, '--steps', '3', '--batch_size', '2', '--segment_size', str(SEGMENT),
              '--checkpoint_interval', '3']
    r = _script(*common, '-o', out, '--second_discriminator', 'mrd')
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert sorted(os.listdir(out)) == ['config.json', 'do_00000003', 'g_00000003', 'vocoder_report.json']
    report = json.load(open(os.path.join(out, 'vocoder_report.json')))
    assert report['second_discriminator'] == 'mrd' and report['steps'] == 3 and report['generator_family'] == 'bigvgan'
    do = torch.load(os.path.join(out, 'do_00000003'), weights_only=False)
    assert sorted(do) == ['epoch', 'mpd', 'mrd', 'optim_d', 'optim_g', 'steps'] and do['steps'] == 3
    assert any(k.startswith('discriminators.1.convs.') for k in do['mrd'])
    do_path, out2 = os.path.join(out, 'do_00000003'), str(tmp_path / 'voc2')
    r = _script(*common, '-g', os.path.join(out, 'g_00000003'), '-do', do_path, '-o', out2, '--second_discriminator', 'mrd')
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    report = json.load(open(os.path.join(out2, 'vocoder_report.json')))
    assert report['first_step'] == 3 and report['steps'] == 6 and 'do_00000006' in os.listdir(out2)
    r = _script(*common, '-do', do_path, '-o', str(tmp_path / 'voc3'), '--second_discriminator', 'msd')
    assert r.returncode != 0 and 'holds an "mrd" entry and no "msd"' in r.stderr and '--second_discriminator mrd' in r.stderr, r.stderr[-2000:]
