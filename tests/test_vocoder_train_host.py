"""Vocoder fine-tuning, the parts that need no GPU: the gradient oracle pinned against plain loops, the data-gradient weight
packings against torch autograd, the discriminators' shapes and names, the losses, the loss mel's reference, the segment sampler,
the checkpoints' layout and the script's argument errors."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vocoder_grad_oracle as G
from tests import vocoder_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T1 = {'resblock': '1', 'upsample_rates': [4, 2], 'upsample_kernel_sizes': [8, 4], 'upsample_initial_channel': 128,
      'resblock_kernel_sizes': [3, 7], 'resblock_dilation_sizes': [[1, 3], [1, 3, 5]], 'num_mels': 80, 'hop_size': 8,
      'sampling_rate': 22050}
MEL_KEYS = {'n_fft': 1024, 'win_size': 1024, 'fmin': 0, 'fmax': 8000, 'fmax_for_loss': None}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the oracle against plain loops ---------------------------------------------------------------------------------------------

def test_conv_oracle_dw_against_a_triple_loop():
    B, C, N, k, d = 2, 2, 5, 3, 2
    g = _gen(1)
    x, dy = torch.randn((B, C, N), generator=g).double(), torch.randn((B, C, N), generator=g).double()
    w, b = torch.randn((C, C, k), generator=g).double(), torch.randn((C,), generator=g).double()
    n = torch.tensor([5, 3])
    x = O.mask_rows(x, n)                                     # the layers' contract: rows at or past n[b] are zeros
    _, dw, db = G.conv_grads(x, w, b, d, n, dy, slope=0.1)
    want, want_b = torch.zeros((C, C, k), dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for bb in range(B):
        for t in range(int(n[bb])):
            for co in range(C):
                want_b[co] += dy[bb, co, t]
                for ci in range(C):
                    for tap in range(k):
                        r = t + (tap - (k - 1) // 2) * d
                        if 0 <= r < int(n[bb]):
                            v = float(x[bb, ci, r])
                            want[co, ci, tap] += dy[bb, co, t] * (v if v > 0 else 0.1 * v)
    assert float((dw - want).abs().max()) < 1e-12 and float((db - want_b).abs().max()) < 1e-12


def test_upsample_oracle_dw_against_a_triple_loop():
    B, C, N, u, k = 2, 2, 5, 3, 7
    pad = (k - u) // 2
    g = _gen(2)
    x, dy = torch.randn((B, C, N), generator=g).double(), torch.randn((B, C, N * u), generator=g).double()
    w, b = torch.randn((C, C, k), generator=g).double(), torch.randn((C,), generator=g).double()
    n = torch.tensor([5, 2])
    x = O.mask_rows(x, n)
    _, dw, _ = G.upsample_grads(x, w, b, u, n, dy, slope=0.1)
    want = torch.zeros((C, C, k), dtype=torch.float64)
    for bb in range(B):
        for t in range(int(n[bb])):                               # y[t u - pad + j] += x[t] w[:, :, j]
            for j in range(k):
                r = t * u - pad + j
                if 0 <= r < int(n[bb]) * u:
                    for ci in range(C):
                        v = float(x[bb, ci, t])
                        for co in range(C):
                            want[ci, co, j] += dy[bb, co, r] * (v if v > 0 else 0.1 * v)
    assert float((dw - want).abs().max()) < 1e-12


def test_round_grad_rounds_dy_but_not_the_bias_gradient():
    g = _gen(3)
    x, dy = torch.randn((1, 2, 6), generator=g).double(), torch.randn((1, 2, 6), generator=g).double()
    w, b, n = torch.randn((2, 2, 3), generator=g).double(), torch.zeros(2).double(), torch.tensor([6])
    _, dw, db = G.conv_grads(x, w, b, 1, n, dy, slope=1., rounding=True)
    _, dw_r, _ = G.conv_grads(O.rnd(x, True), w, b, 1, n, O.rnd(dy, True), slope=1.)
    assert torch.equal(dw, dw_r) and float((db - dy.sum((0, 2))).abs().max()) < 1e-14
    assert not torch.equal(O.rnd(dy, True), dy)


# ---- the data-gradient packings -------------------------------------------------------------------------------------------------

def _conv_rows(x, wp, dilation):
    ''' what dx_voc_conv computes from time-major rows (B, N, Cin) and a packed weight [k][Cout][Cin], in float64 '''
    k = wp.shape[0]
    return F.conv1d(x.transpose(1, 2), wp.permute(1, 2, 0), dilation=dilation, padding=dilation * (k - 1) // 2).transpose(1, 2)


@pytest.mark.parametrize('k,d', [(3, 1), (7, 3), (11, 5)])
def test_conv_dgrad_packing(k, d):
    from daft_exprt.vocoder import pack_conv_dgrad_weight
    g = _gen(k)
    x = torch.randn((2, 5, 40), generator=g).double().requires_grad_(True)
    w, dy = torch.randn((6, 5, k), generator=g).double(), torch.randn((2, 6, 40), generator=g).double()
    y = F.conv1d(x, w, dilation=d, padding=d * (k - 1) // 2)
    want, = torch.autograd.grad((y * dy).sum(), x)
    wd = pack_conv_dgrad_weight(w, torch.float64, 8)
    assert wd.shape == (k, 8, 6) and float(wd[:, 5:].abs().max()) == 0.
    got = _conv_rows(dy.transpose(1, 2), wd, d)
    assert float((got[:, :, :5] - want.transpose(1, 2)).abs().max()) < 1e-12 and float(got[:, :, 5:].abs().max()) == 0.


@pytest.mark.parametrize('u,k', [(8, 16), (2, 4), (4, 8), (3, 7)])
def test_upsample_dgrad_packing(u, k):
    from daft_exprt.vocoder import pack_upsample_dgrad_weight, upsample_dgrad_taps, upsample_tap_table
    g = _gen(u * 100 + k)
    cin, cout, N = 5, 3, 9
    x = torch.randn((2, cin, N), generator=g).double().requires_grad_(True)
    w, dy = torch.randn((cin, cout, k), generator=g).double(), torch.randn((2, cout, N * u), generator=g).double()
    y = F.conv_transpose1d(x, w, stride=u, padding=(k - u) // 2)
    want, = torch.autograd.grad((y * dy).sum(), x)
    wd = pack_upsample_dgrad_weight(w, u, torch.float64)
    taps = upsample_dgrad_taps(k, u)
    assert taps == (5 if (u, k) == (3, 7) else 3) and wd.shape == (taps, cin, u * cout)
    rows = dy.transpose(1, 2).reshape(2, N, u * cout)                      # (B, N u, Cout) read as (B, N, u Cout)
    got = _conv_rows(rows, wd, 1)
    assert float((got - want.transpose(1, 2)).abs().max()) < 1e-12
    j, entry = upsample_tap_table(k, u)                                     # every tap in exactly one entry of the forward's order
    assert sorted(int(v) for v in j.flatten() if v >= 0) == list(range(k))
    assert all(int(j.flatten()[int(entry[t])]) == t for t in range(k))


def test_device_packings_equal_the_host_ones():
    from daft_exprt import vocoder as V
    from daft_exprt import vocoder_train as VT
    g = _gen(5)
    w = torch.randn((6, 5, 7), generator=g).double()
    assert torch.equal(VT.pack_conv_weight(w, torch.float32, 8), V.pack_conv_weight(w, torch.float32, 8))
    for u, k in ((8, 16), (2, 4), (3, 7)):
        wu = torch.randn((5, 3, k), generator=g).double()
        assert torch.equal(VT.pack_upsample_weight(wu, u, torch.bfloat16), V.pack_upsample_weight(wu, u, torch.bfloat16))


# ---- discriminators -------------------------------------------------------------------------------------------------------------

def test_discriminator_shapes_and_names():
    from daft_exprt import vocoder_train as VT
    torch.manual_seed(0)
    mpd, msd = VT.MultiPeriodDiscriminator(), VT.MultiScaleDiscriminator()
    y, y_hat = torch.randn(1, 1, 2048), torch.randn(1, 1, 2048)
    with torch.no_grad():
        real, fake, fmap_r, fmap_g = mpd(y, y_hat)
    assert len(real) == len(fake) == len(fmap_r) == len(fmap_g) == 5
    for p, score, fmap in zip(VT.MPD_PERIODS, real, fmap_r):
        rows = -(-2048 // p)                                                 # reflect-padded to a multiple of the period
        want = []
        for c in (32, 128, 512, 1024):
            rows = (rows + 4 - 5) // 3 + 1
            want.append((1, c, rows, p))
        want += [(1, 1024, rows, p), (1, 1, rows, p)]
        assert [tuple(f.shape) for f in fmap] == want and score.shape == (1, rows * p)
    names = set(mpd.state_dict())
    assert {'discriminators.0.convs.0.weight_g', 'discriminators.0.convs.0.weight_v', 'discriminators.0.convs.0.bias',
            'discriminators.4.conv_post.weight_g'} <= names and len(names) == 5 * 6 * 3
    with torch.no_grad():
        real, fake, fmap_r, _ = msd(y, y_hat)
    assert len(real) == 3
    T = 2048
    for i, (score, fmap) in enumerate(zip(real, fmap_r)):
        if i:
            T = (T + 4 - 4) // 2 + 1
        t, want = T, []
        for _, cout, k, s, _ in VT._MSD_CONVS:
            t = (t + 2 * (k // 2) - k) // s + 1
            want.append((1, cout, t))
        want.append((1, 1, t))
        assert [tuple(f.shape) for f in fmap] == want and score.shape == (1, t)
    names = set(msd.state_dict())
    assert 'discriminators.0.convs.0.weight_orig' in names and 'discriminators.0.convs.0.weight_u' in names       # spectral norm
    assert 'discriminators.1.convs.0.weight_g' in names and 'discriminators.2.conv_post.weight_v' in names


def test_period_padding_at_a_length_that_is_no_multiple_of_the_period():
    from daft_exprt import vocoder_train as VT
    torch.manual_seed(0)
    d = VT.PeriodDiscriminator(11)
    x = torch.arange(2050.).reshape(1, 1, -1)
    seen = []
    d.convs[0].register_forward_pre_hook(lambda mod, inp: seen.append(inp[0]))
    with torch.no_grad():
        d(x)
    folded = seen[0]
    assert folded.shape == (1, 1, 187, 11)                                   # 2050 -> 2057 = 187 x 11
    flat = folded.reshape(-1)
    assert torch.equal(flat[:2050], x[0, 0]) and flat[2050:].tolist() == [2048. - i for i in range(7)]      # reflected, edge excluded


# ---- losses and the loss mel ----------------------------------------------------------------------------------------------------

def test_losses_on_two_element_inputs():
    from daft_exprt import vocoder_train as VT
    real, fake = [torch.tensor([[1., 0.]]), torch.tensor([[0.5, 0.5]])], [torch.tensor([[1., 3.]]), torch.tensor([[0., 2.]])]
    # mean((1 - r)^2): 0.5, 0.25;  mean(g^2): 5, 2
    assert float(VT.discriminator_loss(real, fake)) == pytest.approx(0.5 + 5. + 0.25 + 2.)
    # mean((1 - g)^2): (0 + 4) / 2, (1 + 1) / 2
    assert float(VT.generator_adversarial_loss(fake)) == pytest.approx(2. + 1.)
    fr, fg = [[torch.tensor([1., 2.])], [torch.tensor([0., 0.]), torch.tensor([3., 1.])]], \
             [[torch.tensor([2., 4.])], [torch.tensor([1., -1.]), torch.tensor([3., 0.])]]
    assert float(VT.feature_matching_loss(fr, fg)) == pytest.approx(2. * (1.5 + 1. + 0.5))
    assert float(VT.mel_l1(torch.tensor([[1., 2.]]), torch.tensor([[0., 4.]]))) == pytest.approx(1.5)
    assert VT.MEL_LOSS_WEIGHT == 45.


def test_loss_mel_against_torch_stft():
    from daft_exprt import vocoder_train as VT
    from daft_exprt.extract_features import mel_filter_bank
    cfg = dict(T1, **MEL_KEYS, hop_size=256)
    lm = VT.LossMel(cfg).double()
    g = _gen(7)
    wav = (0.3 * torch.randn((2, 4096), generator=g)).double()
    pad = (1024 - 256) // 2
    spec = torch.stft(F.pad(wav[:, None], (pad, pad), 'reflect')[:, 0], 1024, hop_length=256, win_length=1024,
                      window=torch.hann_window(1024, dtype=torch.float64), center=False, return_complex=True)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    fb = torch.from_numpy(mel_filter_bank(22050, 1024, 80, 0, None)).double()
    want = torch.log(torch.clamp(fb @ mag, min=1e-5))
    got = lm(wav)
    assert got.shape == want.shape == (2, 80, 16)
    assert float((got - want).abs().max()) < 1e-5                            # the basis and the filter bank are held in float32
    with pytest.raises(ValueError, match='fmax_for_loss'):
        VT.LossMel({k: v for k, v in cfg.items() if k != 'fmax_for_loss'})


# ---- the data set ---------------------------------------------------------------------------------------------------------------

def _write_wav(path, pcm, rate=22050):
    data = np.asarray(pcm, dtype='<i2').tobytes()
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 36 + len(data)) + b'WAVE' + b'fmt ' + struct.pack('<IHHIIHH', 16, 1, 1, rate, 2 * rate, 2, 16))
        f.write(b'data' + struct.pack('<I', len(data)) + data)


def _data_set(root, lengths, hop=256, n_mel=80):
    ''' <root>/spk/<i>.npy / .wav: sample i of utterance u is u * 1000 + i // hop, mel[:, t] = u * 1000 + t '''
    os.makedirs(os.path.join(root, 'spk'), exist_ok=True)
    for u, n in enumerate(lengths):
        frames = 1 + n // hop
        np.save(os.path.join(root, 'spk', f'u{u}.npy'), np.tile(u * 1000. + np.arange(frames, dtype=np.float32), (n_mel, 1)))
        _write_wav(os.path.join(root, 'spk', f'u{u}.wav'), u * 1000 + np.arange(n) // hop)


def test_segment_sampler_and_short_pairs(tmp_path):
    from daft_exprt import vocoder_train as VT
    cfg = dict(T1, **MEL_KEYS, hop_size=256)
    root = str(tmp_path / 'ft')
    _data_set(root, [2048 + 700, 1000, 4096, 2048 + 256])
    train, held_out, skipped = VT.read_data_set(root, cfg, 2048, validation_fraction=4)
    assert [name for name, _, _ in train] == ['spk/u0', 'spk/u2'] and skipped == 1            # u1 is shorter than a segment
    assert [name for name, _, _ in held_out] == ['spk/u3']                                    # the 4th by sorted name
    sampler = VT.SegmentSampler(train, 256, 2048, 'cpu', seed=3)
    starts = set()
    for _ in range(40):
        mel, audio = sampler.draw(2)
        assert mel.shape == (2, 80, 8) and audio.shape == (2, 2048)
        for m, a in zip(mel, audio):
            utt, start = int(m[0, 0]) // 1000, int(m[0, 0]) % 1000
            frames = train[[0, None, 1][utt]][1].shape[1]
            assert 0 <= start <= frames - 8 - 1
            assert torch.equal(m[0], utt * 1000. + start + torch.arange(8.))
            assert torch.equal(a * 32768., (utt * 1000. + start + torch.arange(2048) // 256).float())    # the same frames' samples
            starts.add((utt, start))
    assert {s for u, s in starts if u == 0} == {0, 1, 2} and len({s for u, s in starts if u == 2}) > 4
    assert sampler.epoch == 40
    with pytest.raises(ValueError, match='multiple of the hop'):
        VT.SegmentSampler(train, 256, 2000, 'cpu')


def test_frame_count_mismatch_names_the_file(tmp_path):
    from daft_exprt import vocoder_train as VT
    cfg = dict(T1, **MEL_KEYS, hop_size=256)
    root = str(tmp_path / 'ft')
    _data_set(root, [4096])
    np.save(os.path.join(root, 'spk', 'u0.npy'), np.zeros((80, 16), dtype=np.float32))          # 4096 samples give 17 frames
    with pytest.raises(ValueError, match=r'u0\.npy: 16 frames.*4096 samples gives 17'):
        VT.read_data_set(root, cfg, 2048)


# ---- the generator's parameters and the checkpoints -----------------------------------------------------------------------------

def _weights(cfg, seed=0):
    lengths = (3,)
    mel = O.make_mel(cfg, lengths, seed=seed)
    return O.make_weights(cfg, mel, lengths, seed=seed)


@pytest.mark.parametrize('form', O.FORMS)
def test_trainable_generator_state_round_trips(form):
    from daft_exprt import vocoder as V
    from daft_exprt import vocoder_train as VT
    weights = _weights(T1)
    gen = VT.TrainableGenerator(T1, O.state_dict(weights, form))
    sd = gen.state_dict()
    names = [n for n, _, _, _ in V.layer_table(T1)]
    assert sorted(sd) == sorted(f'{n}{s}' for n in names for s in ('.weight_g', '.weight_v', '.bias'))
    assert [n for n, _ in gen.named_parameters()] == list(sd)
    folded = V.folded_state(T1, sd)
    for name, (w, b) in weights.items():
        assert float((folded[name][0] - w.double()).abs().max()) <= 4e-7 * float(w.abs().max()), name
        assert torch.equal(folded[name][1], b.double())
    if form != 'plain':                                     # g and v are kept as the checkpoint holds them
        src = O.state_dict(weights, form)
        g_key = 'conv_pre.weight_g' if form == 'weight_norm' else 'conv_pre.parametrizations.weight.original0'
        assert torch.equal(sd['conv_pre.weight_g'], src[g_key])


def test_v2_tail_is_rejected_naming_the_stage():
    from daft_exprt import vocoder_train as VT
    weights = _weights(O.SMALL)
    with pytest.raises(ValueError, match=r'"ups\.1" has 16 channels.*multiple of 32'):
        VT.TrainableGenerator(O.SMALL, O.state_dict(weights))
    with pytest.raises(ValueError, match='compute_dtype'):
        VT.TrainableGenerator(T1, O.state_dict(_weights(T1)), compute_dtype='fp16')


def test_checkpoint_layout_and_foreign_do_files(tmp_path):
    from daft_exprt import vocoder as V
    from daft_exprt import vocoder_train as VT
    torch.manual_seed(0)
    gen = VT.TrainableGenerator(T1, O.state_dict(_weights(T1), 'weight_norm'))

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv1d(1, 1, 3)
    mpd, msd = Tiny(), Tiny()
    og, od = torch.optim.AdamW(gen.parameters(), 2e-4, betas=(0.8, 0.99)), torch.optim.AdamW(list(msd.parameters()) + list(mpd.parameters()))
    g_path, do_path = VT.save_checkpoints(str(tmp_path), T1, gen, mpd, msd, og, od, 12, 3)
    assert os.path.basename(g_path) == 'g_00000012' and os.path.basename(do_path) == 'do_00000012'
    assert json.load(open(tmp_path / 'config.json')) == T1
    g = torch.load(g_path, weights_only=False)
    assert list(g) == ['generator'] and sorted(g['generator']) == sorted(gen.state_dict())
    V.folded_state(T1, g['generator'])                                       # what Vocoder.from_checkpoint reads
    do = torch.load(do_path, weights_only=False)
    assert sorted(do) == ['epoch', 'mpd', 'msd', 'optim_d', 'optim_g', 'steps'] and do['steps'] == 12 and do['epoch'] == 3
    assert VT.load_discriminator_state(do_path, Tiny(), Tiny()) == (12, 3)
    del do['mpd']['conv.bias']
    torch.save(do, do_path)
    with pytest.raises(ValueError, match='"mpd" has no "conv.bias"'):
        VT.load_discriminator_state(do_path, Tiny(), Tiny())
    torch.save({'generator': {}}, do_path)
    with pytest.raises(ValueError, match='no "mpd" entry'):
        VT.load_discriminator_state(do_path, Tiny(), Tiny())


def test_new_entry_points_are_declared_and_exported():
    from daft_exprt import _hip as H
    protos = {name: args for name, _, args in H.header_prototypes()}
    assert len(protos['dx_vocoder_wgrad']) == 16 and len(protos['dx_vocoder_upsample_wgrad']) == 16 and len(protos['dx_vocoder_wgrad_workspace']) == 6
    if os.path.exists(H.LIB_PATH):
        lib = H.lib()
        assert lib.dx_abi_version() == 13
        assert lib.dx_vocoder_wgrad_workspace(3, 257, 64, 32, 7, 1) > 0 and lib.dx_vocoder_wgrad_workspace(0, 257, 64, 32, 7, 1) == 0
        # refusals come before any launch: channel counts, tap span
        assert lib.dx_vocoder_wgrad(1, 16, 1, 16, H.F32, 1, 1, 1, 1, 8, 16, 16, 3, 1, 0.1, None) == -5
        assert b'multiples of 32' in lib.dx_last_error()
        assert lib.dx_vocoder_wgrad(1, 32, 1, 32, H.F32, 1, 1, 1, 1, 8, 32, 32, 15, 5, 0.1, None) == -5
        assert b'span 70 rows' in lib.dx_last_error()


# ---- the script -----------------------------------------------------------------------------------------------------------------

def _run_script(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'train_vocoder.py'), *args], capture_output=True, text=True,
                          timeout=120)


def test_script_argument_errors(tmp_path):
    root = str(tmp_path / 'ft')
    _data_set(root, [4096])
    cfg = dict(T1, **MEL_KEYS, upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512, hop_size=256)
    cfg_path, g_path, out = str(tmp_path / 'config.json'), str(tmp_path / 'g_00000000'), str(tmp_path / 'out')
    json.dump(cfg, open(cfg_path, 'w'))
    open(g_path, 'wb').close()
    ok = ['-ft', root, '-cfg', cfg_path, '-g', g_path, '-o', out]

    def fails(args, text):
        r = _run_script(*args)
        assert r.returncode != 0 and text in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr[-2000:]
    fails(['-ft', root + '_none'] + ok[2:], 'no such fine-tuning data set')
    fails(ok[:3] + [cfg_path + '_none'] + ok[4:], 'no such config')
    fails(ok[:5] + [g_path + '_none'] + ok[6:], 'no such generator checkpoint')
    fails(ok + ['-do', str(tmp_path / 'do_none')], 'no such discriminator checkpoint')
    fails(ok + ['--steps', '0'], 'must be at least 1')
    fails(ok + ['--segment_size', '2000'], 'not a multiple of the config\'s hop_size 256')
    v2 = str(tmp_path / 'v2.json')
    json.dump(dict(cfg, upsample_initial_channel=128), open(v2, 'w'))
    fails(ok[:3] + [v2] + ok[4:], 'multiple of 32')
    no_mel = str(tmp_path / 'no_mel.json')
    json.dump({k: v for k, v in cfg.items() if k != 'win_size'}, open(no_mel, 'w'))
    fails(ok[:3] + [no_mel] + ok[4:], '"win_size" is missing')
