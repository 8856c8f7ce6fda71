"""Host side of K36 (the magnitude spectrogram and its gradient) and of the multi-resolution discriminator: tests/spectrogram_oracle.py
against `torch.stft` + `torch.norm` + autograd in float64, the backward's index sums against that autograd, silence, the frame count,
the entry points' refusals (returned before any launch: no GPU is needed), the discriminator's names and shapes through the oracle
hook, the `do_` layout with `mrd`, the script's flag, and the conditioning of every gradient case of tests/test_gpu_spectrogram.py."""
import ctypes
import json
import os

import pytest
import torch

from tests import spectrogram_oracle as SO

pytestmark = pytest.mark.filterwarnings('ignore:A window was not provided')      # window=None is upstream's call, restated on purpose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _stft_mag(x, n_fft, hop, win):
    ''' upstream's `DiscriminatorR.spectrogram` on one utterance, float64: (bins, F) '''
    p = int((n_fft - hop) / 2)
    padded = torch.nn.functional.pad(x[None, None], (p, p), mode='reflect')[0]
    spec = torch.stft(padded, n_fft=n_fft, hop_length=hop, win_length=win, window=None, center=False, return_complex=True)
    return torch.norm(torch.view_as_real(spec), p=2, dim=-1)[0]


def _lengths(n_fft, hop):
    p = (n_fft - hop) // 2
    return (p + 1, p + 2, 2 * p + 1, 4113)


@pytest.mark.parametrize('resolution', SO.RESOLUTIONS)
def test_oracle_against_torch_stft_and_autograd(resolution):
    n_fft, hop, win = resolution
    for i, n in enumerate(_lengths(n_fft, hop)):
        g = _gen(10 * n_fft + i)
        x = torch.randn((n,), generator=g, dtype=torch.float64)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        want = _stft_mag(xa, n_fft, hop, win)
        got = SO.magnitude(xb, n_fft, hop, SO.window_table(n_fft, win))
        assert got.shape == want.shape == (n_fft // 2 + 1, SO.frames_of(n, n_fft, hop))
        proj = torch.randn(want.shape, generator=g, dtype=torch.float64)
        dwant, = torch.autograd.grad((want * proj).sum(), xa)
        dgot, = torch.autograd.grad((got * proj).sum(), xb)
        e_f = float((got - want).detach().abs().max() / want.detach().abs().max())
        e_g = float((dgot - dwant).abs().max() / dwant.abs().max())
        print(f'{resolution} n {n}: forward {e_f:.3g}, gradient {e_g:.3g} (relative)')
        assert e_f <= 1e-10 and e_g <= 1e-10, (n, e_f, e_g)
        sums = SO.backward_index_sums(x, proj, n_fft, hop, SO.window_table(n_fft, win))
        e_s = float((sums - dwant).abs().max() / dwant.abs().max())
        print(f'{resolution} n {n}: index sums {e_s:.3g} (relative)')
        assert e_s <= 1e-10, (n, e_s)


def test_batched_oracle_is_each_utterance_alone_with_zeros_past_its_end():
    name = '512-50-240-b'
    n_fft, hop, window, n, wav, dmag = SO.case_inputs(name)
    garbage = wav.clone()
    for b, k in enumerate(n):
        garbage[b, k:] = float('nan')
    mag, dwav = SO.spectrogram(garbage, n, n_fft, hop, window, dmag=dmag)
    assert bool(torch.isfinite(mag).all()) and bool(torch.isfinite(dwav).all())
    for b, k in enumerate(n):
        f = SO.frames_of(k, n_fft, hop)
        alone = SO.magnitude(wav[b, :k], n_fft, hop, window)
        assert torch.equal(mag[b, :, :f], alone) and float(mag[b, :, f:].abs().sum()) == 0. and float(dwav[b, k:].abs().sum()) == 0.


def test_silence_gives_a_finite_gradient_and_silent_frames_give_none():
    n_fft, hop, win = 512, 50, 240
    w = SO.window_table(n_fft, win)
    zero = torch.zeros((1, 700), dtype=torch.float64)
    mag, dwav = SO.spectrogram(zero, [700], n_fft, hop, w, dmag=torch.ones((1, 257, SO.frames_of(700, n_fft, hop)), dtype=torch.float64))
    assert float(mag.abs().max()) == 0. and float(dwav.abs().max()) == 0.
    assert float(SO.backward_index_sums(zero[0], torch.ones((257, SO.frames_of(700, n_fft, hop)), dtype=torch.float64), n_fft, hop, w).abs().max()) == 0.
    # digital silence over [1000, 2000), longer than n_fft: the frames wholly inside it have |X| = 0 and contribute nothing
    x = torch.randn((3000,), generator=_gen(3), dtype=torch.float64)
    x[1000:2000] = 0.
    p, frames = (n_fft - hop) // 2, SO.frames_of(3000, n_fft, hop)
    silent = [f for f in range(frames) if f * hop - p >= 1000 and f * hop - p + n_fft <= 2000]
    assert len(silent) >= 5
    proj = torch.randn((257, frames), generator=_gen(4), dtype=torch.float64)
    xa = x.clone().requires_grad_(True)
    m = SO.magnitude(xa, n_fft, hop, w)
    grad, = torch.autograd.grad((m * proj).sum(), xa)
    assert bool(torch.isfinite(grad).all()) and float(m.detach()[:, silent].abs().max()) == 0.
    without = proj.clone()
    without[:, silent] = 0.
    xb = x.clone().requires_grad_(True)
    other, = torch.autograd.grad((SO.magnitude(xb, n_fft, hop, w) * without).sum(), xb)
    assert torch.equal(grad, other)                                          # the silent frames' own contribution is zero
    assert torch.allclose(SO.backward_index_sums(x, proj, n_fft, hop, w), grad, rtol=0, atol=1e-10 * float(grad.abs().max()))
    # samples that only silent frames cover get no gradient at all
    covered = [i for i in range(1000, 2000) if all(f in silent for f in range(frames) if 0 <= i - (f * hop - p) < n_fft)]
    assert covered and float(grad[covered].abs().max()) == 0.


def test_spectrogram_frames():
    from daft_exprt.spectrogram import rectangular_window, spectrogram_frames
    for n_fft, hop, win in SO.RESOLUTIONS:
        p = (n_fft - hop) // 2
        for n in (p + 1, 2 * p + 1, 4113, 8192):
            x = torch.zeros((n,), dtype=torch.float64)
            assert spectrogram_frames(n, n_fft, hop) == _stft_mag(x, n_fft, hop, win).shape[1] == SO.frames_of(n, n_fft, hop)
        with pytest.raises(ValueError, match='too few'):
            spectrogram_frames(p, n_fft, hop)
        with pytest.raises(RuntimeError):                                    # torch refuses the same padding
            _stft_mag(torch.zeros((p,), dtype=torch.float64), n_fft, hop, win)
        assert torch.equal(rectangular_window(n_fft, win).double(), SO.window_table(n_fft, win))
    assert [spectrogram_frames(8192, *r[:2]) for r in SO.RESOLUTIONS] == [68, 34, 163]       # x 16 = 1 088 / 544 / 2 608 per batch
    assert spectrogram_frames(232, 512, 50) == 4 and spectrogram_frames(453, 1024, 120) == 3 and spectrogram_frames(905, 2048, 240) == 3
    with pytest.raises(ValueError, match='hop'):
        spectrogram_frames(4000, 512, 0)
    with pytest.raises(ValueError, match='hop'):
        spectrogram_frames(4000, 512, 513)


def _lib():
    from daft_exprt import _hip as H
    if not os.path.exists(H.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return H, H.lib()


def test_entry_points_are_declared_exported_and_refuse_before_any_launch():
    H, lib = _lib()
    protos = {name: args for name, _, args in H.header_prototypes()}
    new = ['dx_spectrogram', 'dx_spectrogram_bwd', 'dx_spectrogram_bwd_workspace', 'dx_spectrogram_tables']
    assert sorted(k for k in protos if k.startswith('dx_spectrogram')) == new
    assert [len(protos[k]) for k in new] == [13, 16, 3, 3]
    for name in new:
        assert hasattr(lib, name), f'{name} declared in include/daft_exprt_hip.h but not exported'
    assert lib.dx_abi_version() == 13
    assert lib.dx_spectrogram_bwd_workspace(3, 82, 512) == 3 * 82 * 512 * 4 and lib.dx_spectrogram_bwd_workspace(0, 82, 512) == 0
    assert lib.dx_spectrogram_bwd_workspace(16, 35, 2048) == 16 * 35 * 2048 * 4

    def host(*n):
        return (ctypes.c_int64 * len(n))(*n)
    ok = host(700, 4113)

    def fwd(wav=1, nd=1, nh=ok, tw=1, win=1, mag=1, B=2, S=4113, T=82, n_fft=512, hop=50):
        return lib.dx_spectrogram(wav, S, nd, ctypes.addressof(nh) if nh is not None else None, tw, win, mag, B, S, T, n_fft, hop, None)

    def bwd(wav=1, nd=1, nh=ok, tw=1, win=1, dmag=1, dwav=1, ws=1, B=2, S=4113, T=82, n_fft=512, hop=50):
        return lib.dx_spectrogram_bwd(wav, S, nd, ctypes.addressof(nh) if nh is not None else None, tw, win, dmag, dwav, S, ws, B, S, T, n_fft,
                                      hop, None)
    for call in (fwd, bwd):
        assert call(wav=None) == -1 and b'null' in lib.dx_last_error()
        assert call(nh=None) == -1 and b'null' in lib.dx_last_error()
        for bad in (2048 + 1, 128, 8192, 768, 0):
            assert call(n_fft=bad) == -5 and b'n_fft' in lib.dx_last_error(), bad
        assert call(hop=0) == -5 and b'hop' in lib.dx_last_error()
        assert call(hop=513) == -5 and b'hop' in lib.dx_last_error()
        assert call(nh=host(700, 231)) == -5 and b'utterance 1 has 231 samples' in lib.dx_last_error()      # n = p
        assert call(nh=host(0, 700)) == -5 and b'utterance 0 has 0 samples' in lib.dx_last_error()
        assert call(nh=host(700, 5000)) == -2 and b'utterance 1' in lib.dx_last_error()                     # past the row
        assert call(T=81) == -2 and b'utterance 1 has 82 frames' in lib.dx_last_error()
        assert call(B=0) == -2
    assert bwd(ws=None) == -1 and bwd(dwav=None) == -1 and fwd(mag=None) == -1
    # hop = n_fft: p = 0, one sample is not enough for a frame
    assert fwd(nh=host(255, 4113), n_fft=256, hop=256, T=100) == -5 and b'utterance 0' in lib.dx_last_error()
    assert lib.dx_spectrogram_tables(None, 512, None) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_spectrogram_tables(1, 768, None) == -5 and b'n_fft' in lib.dx_last_error()
    # the front end's and Griffin-Lim's sizes are untouched
    assert lib.dx_mel_tables(1, 1, 2048, None) == -1 and lib.dx_mel_tables(1, 1, 512, None) == -1


def test_python_wrapper_refuses_on_the_host():
    from daft_exprt.spectrogram import spectrogram
    with pytest.raises(RuntimeError, match='device tensors'):
        spectrogram(torch.zeros((1, 4000)), [4000], 512, 50)


# ---- the discriminator -----------------------------------------------------------------------------------------------------------

def _oracle_hook(wav, n_fft, hop, win):
    return torch.stack([SO.magnitude(wav[b], n_fft, hop, SO.window_table(n_fft, win, wav.dtype)) for b in range(wav.shape[0])])


def test_mrd_names_shapes_and_the_short_segment_error():
    from daft_exprt import bigvgan_train as BT
    torch.manual_seed(0)
    mrd = BT.MultiResolutionDiscriminator(spectrogram=_oracle_hook)
    assert [d.resolution for d in mrd.discriminators] == [(1024, 120, 600), (2048, 240, 1200), (512, 50, 240)]
    keys = sorted(mrd.state_dict())
    want = sorted(f'discriminators.{n}.{m}.{part}' for n in range(3) for m in [f'convs.{i}' for i in range(5)] + ['conv_post']
                  for part in ('bias', 'weight_g', 'weight_v'))
    assert keys == want
    sd = mrd.state_dict()
    assert sd['discriminators.0.convs.0.weight_v'].shape == (32, 1, 3, 9) and sd['discriminators.0.convs.1.weight_v'].shape == (32, 32, 3, 9)
    assert sd['discriminators.2.convs.4.weight_v'].shape == (32, 32, 3, 3) and sd['discriminators.1.conv_post.weight_v'].shape == (1, 32, 3, 3)
    assert [c.stride for c in mrd.discriminators[0].convs] == [(1, 1), (1, 2), (1, 2), (1, 2), (1, 1)]
    y, y_hat = torch.randn((2, 1, 2048), generator=_gen(1)), torch.randn((2, 1, 2048), generator=_gen(2)).requires_grad_(True)
    real, fake, fmap_r, fmap_g = mrd(y, y_hat)
    assert len(real) == len(fake) == len(fmap_r) == len(fmap_g) == 3
    for d, score, fmap in zip(mrd.discriminators, fake, fmap_g):
        n_fft, hop, _ = d.resolution
        bins, t = n_fft // 2 + 1, SO.frames_of(2048, n_fft, hop)
        widths = [t]
        for _ in range(3):
            widths.append((widths[-1] + 2 * 4 - 9) // 2 + 1)
        assert [tuple(f.shape) for f in fmap] == [(2, 32, bins, w) for w in widths + [widths[-1]]] + [(2, 1, bins, widths[-1])]
        assert score.shape == (2, bins * widths[-1])
    sum(s.sum() for s in fake).backward()
    assert bool(torch.isfinite(y_hat.grad).all()) and float(y_hat.grad.abs().max()) > 0.
    # the module against the oracle's functional form on the same weights
    d = mrd.discriminators[2]
    weights = {k: v.double() for k, v in d.state_dict().items()}
    scores, fmaps = SO.discriminator_r(weights, y[:, 0], d.resolution, dtype=torch.float32)
    got, got_maps = d(y)
    assert torch.allclose(got, scores, rtol=1e-4, atol=1e-5) and all(torch.allclose(a, b, rtol=1e-4, atol=1e-5) for a, b in zip(got_maps, fmaps))
    wide = BT.MultiResolutionDiscriminator({'resolutions': [[256, 64, 256]], 'discriminator_channel_mult': 2, 'use_spectral_norm': True},
                                           spectrogram=_oracle_hook)
    assert wide.discriminators[0].convs[1].weight.shape == (64, 64, 3, 9) and 'discriminators.0.convs.0.weight_orig' in wide.state_dict()
    with pytest.raises(ValueError, match=r'too short for the resolution \(n_fft 2048, hop 240, win 1200\)'):
        mrd(torch.zeros((1, 1, 904)), torch.zeros((1, 1, 904)))
    with pytest.raises(ValueError, match='n_fft 2048'):
        mrd.check_segment(600)
    mrd.check_segment(905)


def test_do_round_trip_with_mrd_and_the_wrong_kind(tmp_path):
    from daft_exprt import bigvgan_train as BT
    from daft_exprt import vocoder_train as VT

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv1d(1, 1, 3)

    torch.manual_seed(0)
    gen, mpd = Tiny(), Tiny()
    mrd = BT.MultiResolutionDiscriminator({'resolutions': [[256, 64, 256]]}, spectrogram=_oracle_hook)
    og, od = torch.optim.AdamW(gen.parameters()), torch.optim.AdamW(list(mrd.parameters()) + list(mpd.parameters()))
    _, do_path = VT.save_checkpoints(str(tmp_path), {'a': 1}, gen, mpd, mrd, og, od, 7, 2, second='mrd')
    do = torch.load(do_path, weights_only=False)
    assert sorted(do) == ['epoch', 'mpd', 'mrd', 'optim_d', 'optim_g', 'steps']
    assert sorted(do['mrd']) == sorted(mrd.state_dict())
    fresh = BT.MultiResolutionDiscriminator({'resolutions': [[256, 64, 256]]}, spectrogram=_oracle_hook)
    assert VT.load_discriminator_state(do_path, Tiny(), fresh, second='mrd') == (7, 2)
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), mrd.state_dict().values()))
    with pytest.raises(ValueError, match=r'holds an "mrd" entry and no "msd".*--second_discriminator mrd'):
        VT.load_discriminator_state(do_path, Tiny(), Tiny())
    _, msd_path = VT.save_checkpoints(str(tmp_path / 'msd'), {'a': 1}, gen, mpd, Tiny(), og, od, 9, 1)
    assert 'msd' in torch.load(msd_path, weights_only=False)
    with pytest.raises(ValueError, match=r'holds an "msd" entry and no "mrd".*--second_discriminator msd'):
        VT.load_discriminator_state(msd_path, Tiny(), fresh, second='mrd')
    torch.save({'mpd': {}, 'optim_g': {}}, do_path)                          # neither kind: the message of a missing key stays
    with pytest.raises(ValueError, match='no "msd" entry'):
        VT.load_discriminator_state(do_path, Tiny(), Tiny())
    with pytest.raises(ValueError, match='no "mrd" entry'):
        VT.load_discriminator_state(do_path, Tiny(), fresh, second='mrd')
    with pytest.raises(ValueError, match='second_discriminator'):
        VT.save_checkpoints(str(tmp_path), {'a': 1}, gen, mpd, mrd, og, od, 7, 2, second='cqt')


def test_script_flag_parses():
    import importlib.util
    spec = importlib.util.spec_from_file_location('train_vocoder_script', os.path.join(ROOT, 'scripts', 'train_vocoder.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ['-ft', 'a', '-cfg', 'b', '-g', 'c', '-o', 'd']
    assert mod.parse_args(base).second_discriminator == 'msd'
    assert mod.parse_args(base + ['--second_discriminator', 'mrd']).second_discriminator == 'mrd'
    with pytest.raises(SystemExit):
        mod.parse_args(base + ['--second_discriminator', 'cqt'])


def test_fine_tune_vocoder_refuses_an_unknown_second_discriminator():
    from daft_exprt import vocoder_train as VT
    import inspect
    assert inspect.signature(VT.fine_tune_vocoder).parameters['second_discriminator'].default == 'msd'
    assert inspect.signature(VT.train_step).parameters['clip_grad_norm'].default is None
    assert (VT.MRD_LEARNING_RATE, VT.MRD_CLIP_GRAD_NORM) == (1e-4, 1000.)


# ---- the GPU file's gradient cases are well conditioned -----------------------------------------------------------------------------

@pytest.mark.parametrize('name', [c[0] for c in SO.CASES])
def test_gpu_gradient_cases_are_well_conditioned(name):
    ''' X / |X| is ill-conditioned near a zero of X: over the live bins and frames of every utterance, min |X| >= 1e-3 max |X| '''
    ratio = SO.case_condition(name)
    print(f'{name}: min |X| / max |X| = {ratio:.3g}')
    assert ratio >= SO.CONDITION


@pytest.mark.parametrize('resolution', SO.RESOLUTIONS)
def test_gpu_module_cases_are_well_conditioned(resolution):
    ratio = SO.module_condition(resolution)
    print(f'{resolution}: min |X| / max |X| = {ratio:.3g}')
    assert ratio >= SO.CONDITION


def test_gpu_cases_cover_the_lengths_and_sizes():
    seen = set()
    for _, n_fft, hop, win, n in SO.CASES:
        seen.add(n_fft)
        assert len(n) == 3 and len(set(n)) == 3
    assert seen == {256, 512, 1024, 2048, 4096}
    for n_fft, hop, win in SO.RESOLUTIONS:
        p = (n_fft - hop) // 2
        lengths = {k for c in SO.CASES if c[1:4] == (n_fft, hop, win) for k in c[4]}
        assert {p + 1, 2 * p + 1, 4113} <= lengths
        assert any((k + 2 * p - n_fft) % hop == hop - 1 for k in lengths)
    assert json.dumps(sorted(SO.SEEDS)) == json.dumps(sorted(c[0] for c in SO.CASES))
