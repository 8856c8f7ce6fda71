"""The HiFi-GAN vocoder (K24: csrc/vocoder.hip, daft_exprt/vocoder.py) on the GPU against tests/vocoder_oracle.py -- the float64
restatement pinned in tests/test_vocoder_host.py -- and never against the code under test.

Tolerances are computed at run time from the oracle's own switches (no constants beyond the floors):
    fp32   max |y - oracle64| <= max(8 x max |oracle32 - oracle64|, 2e-6): the float32 CPU run of the same restatement measures what
           fp32 arithmetic costs on this input; the factor 8 covers the other summation order (a k-ordered fmaf chain in the MFMA)
    bf16   the project's stage rule: with d_round = max |oracle_rounded - oracle64| (operands rounded to bf16, float64 sums),
           max |y - oracle_rounded| <= max(2 d_round, 2e-3)
Every test prints the measured values.  Shapes: one 256-row tile + 1, an utterance shorter than the halo, a single row."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import vocoder_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (257, 3, 1)
DTYPES = ['fp32', 'bf16']


def _bound(y, o64, o32, o_rounded, dtype, what):
    ''' asserts the module's tolerance rule on CPU float64 tensors of one shape '''
    y = y.double().cpu()
    assert y.shape == o64.shape, (y.shape, o64.shape)
    assert bool(torch.isfinite(y).all()), what
    if dtype == 'fp32':
        cost = float((o32.double() - o64).abs().max())
        err, tol = float((y - o64).abs().max()), max(8. * cost, 2e-6)
        print(f'{what} fp32: err {err:.3g}, fp32 oracle cost {cost:.3g}, bound {tol:.3g}')
    else:
        d_round = float((o_rounded - o64).abs().max())
        err, tol = float((y - o_rounded).abs().max()), max(2. * d_round, 2e-3)
        print(f'{what} bf16: err vs rounded oracle {err:.3g}, d_round {d_round:.3g}, bound {tol:.3g}')
    assert err <= tol, (what, dtype, err, tol)


def _three(fn):
    ''' (oracle64, oracle32, oracle_rounded) of fn(dtype, rounding) '''
    return fn(torch.float64, False), fn(torch.float32, False), fn(torch.float64, True)


def _rows_major(x, n=None):
    ''' (B, C, T) CPU -> (B, T, C) fp32 on the device; with `n` the rows at or past n[b] are NaN: they must not be read '''
    x = x.float().transpose(1, 2).contiguous()
    if n is not None:
        for b, rows in enumerate(n):
            x[b, rows:] = float('nan')
    return x.to(DEV)


def _wdt(dtype):
    from daft_exprt import _hip as H
    return (torch.bfloat16, H.BF16) if dtype == 'bf16' else (torch.float32, H.F32)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- each kernel alone ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('fused', [False, True], ids=['plain', 'residual_accumulate'])
@pytest.mark.parametrize('cin,cout', [(32, 32), (64, 32), (96, 64), (16, 16), (80, 64)])
def test_conv_alone(cin, cout, fused, dtype):
    from daft_exprt import _hip as H
    from daft_exprt.vocoder import pack_conv_weight
    tdt, wdt = _wdt(dtype)
    B, N, n = len(ROWS), max(ROWS), torch.tensor(ROWS)
    g = _gen(cin * 100 + cout)
    x = O.mask_rows(torch.randn((B, cin, N), generator=g), n)
    res = O.mask_rows(torch.randn((B, cout, N), generator=g), n)
    xd, rd, nd = _rows_major(x, n=ROWS), _rows_major(res, n=ROWS), n.to(DEV)
    for k in (3, 7, 11):
        for d in (1, 3, 5):
            w = torch.randn((cout, cin, k), generator=g) / (cin * k) ** 0.5
            bias = 0.1 * torch.randn((cout,), generator=g)
            wp = pack_conv_weight(w.double(), tdt).to(DEV)
            bd = bias.to(DEV)

            def ref(dt, rounding):
                v = O.conv(x.to(dt), w, bias, d, n, slope=0.1, rounding=rounding)
                return (O.mask_rows(v + res.to(dt), n) if fused else v).double().transpose(1, 2)
            o64, o32, orr = _three(ref)
            y = torch.full((B, N, cout), float('nan'), device=DEV)
            acc = torch.full((B, N, cout), float('nan'), device=DEV) if fused else None
            H.check(H.lib().dx_voc_conv(H.ptr(xd), cin, H.ptr(wp), wdt, H.ptr(bd), H.ptr(rd) if fused else None, cout, H.ptr(y), cout,
                                        H.ptr(acc), cout, 0.5, 1, H.ptr(nd), B, N, cin, cout, k, d, 0.1, H.stream()))
            _bound(y, o64, o32, orr, dtype, f'conv {cin}->{cout} k{k} d{d}')
            for b, rows in enumerate(ROWS):
                assert float(y[b, rows:].abs().max() if rows < N else 0.) == 0.                  # dead rows: exact zeros
            if fused:                                                                          # the running ResBlock sum
                _bound(acc, 0.5 * o64, 0.5 * o32, 0.5 * orr, dtype, '  acc (init)')
                H.check(H.lib().dx_voc_conv(H.ptr(xd), cin, H.ptr(wp), wdt, H.ptr(bd), H.ptr(rd), cout, None, cout, H.ptr(acc), cout,
                                            0.25, 0, H.ptr(nd), B, N, cin, cout, k, d, 0.1, H.stream()))
                _bound(acc, 0.75 * o64, 0.75 * o32, 0.75 * orr, dtype, '  acc (accumulate)')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cin,cout,k,d', [(96, 64, 3, 3), (64, 32, 11, 5), (32, 32, 7, 1), (16, 16, 3, 1)])
def test_conv_lane_maps_with_asymmetric_integers(cin, cout, k, d, dtype):
    ''' small integers are exact in bf16 and their sums exact in fp32: any lane, tap or channel mix-up changes the result,
        and the operands are symmetric in no pair of indices '''
    from daft_exprt import _hip as H
    from daft_exprt.vocoder import pack_conv_weight
    tdt, wdt = _wdt(dtype)
    B, N, n = len(ROWS), max(ROWS), torch.tensor(ROWS)
    t, c, o, j = torch.arange(N), torch.arange(cin), torch.arange(cout), torch.arange(k)
    x = (((3 * t[None, :] + 5 * c[:, None]) % 7) - 3).double()[None].repeat(B, 1, 1) + torch.arange(B).double()[:, None, None]
    x = O.mask_rows(x, n)
    w = (((2 * o[:, None, None] + 3 * c[None, :, None] + 5 * j[None, None, :]) % 5) - 2).double()
    bias = (o % 3).double()
    want = O.conv(x, w, bias, d, n, slope=1.).transpose(1, 2)
    y = torch.full((B, N, cout), float('nan'), device=DEV)
    xd, wp, bd, nd = _rows_major(x, n=ROWS), pack_conv_weight(w, tdt).to(DEV), bias.float().to(DEV), n.to(DEV)
    H.check(H.lib().dx_voc_conv(H.ptr(xd), cin, H.ptr(wp), wdt, H.ptr(bd), None, cout, H.ptr(y), cout, None, cout, 0., 0, H.ptr(nd), B, N,
                                cin, cout, k, d, 1., H.stream()))
    assert torch.equal(y.double().cpu(), want)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cin,cout', [(64, 32), (16, 8)])
@pytest.mark.parametrize('u,k', [(8, 16), (2, 4), (4, 8), (3, 7)])
def test_upsample_alone(u, k, cin, cout, dtype):
    from daft_exprt import _hip as H
    from daft_exprt.vocoder import pack_upsample_weight
    tdt, wdt = _wdt(dtype)
    B, N, n = len(ROWS), max(ROWS), torch.tensor(ROWS)
    g = _gen(u * 1000 + k * 10 + cin)
    x = O.mask_rows(torch.randn((B, cin, N), generator=g), n)
    w = torch.randn((cin, cout, k), generator=g) / (cin * k / u) ** 0.5
    bias = 0.1 * torch.randn((cout,), generator=g)
    o64, o32, orr = _three(lambda dt, rounding: O.upsample(x.to(dt), w, bias, u, n, rounding=rounding).double().transpose(1, 2))
    y = torch.full((B, N * u, cout), float('nan'), device=DEV)
    xd, wp, bd, nd = _rows_major(x, n=ROWS), pack_upsample_weight(w.double(), u, tdt).to(DEV), bias.to(DEV), n.to(DEV)
    H.check(H.lib().dx_voc_upsample(H.ptr(xd), cin, H.ptr(wp), wdt, H.ptr(bd), H.ptr(y), cout, H.ptr(nd), B, N, cin, cout, k, u, 0.1,
                                    H.stream()))
    _bound(y, o64, o32, orr, dtype, f'upsample {cin}->{cout} u{u} k{k}')
    for b, rows in enumerate(ROWS):
        assert float(y[b, rows * u:].abs().max() if rows < N else 0.) == 0.
    # integers: every phase takes its own taps from its own input rows
    t, c, o, j = torch.arange(N), torch.arange(cin), torch.arange(cout), torch.arange(k)
    xi = O.mask_rows((((3 * t[None, :] + 5 * c[:, None]) % 7) - 3).double()[None].repeat(B, 1, 1), n)
    wi = (((2 * c[:, None, None] + 3 * o[None, :, None] + 5 * j[None, None, :]) % 5) - 2).double()
    want = O.upsample(xi, wi, torch.zeros(cout, dtype=torch.float64), u, n, slope=1.).transpose(1, 2)
    xd, wp = _rows_major(xi, n=ROWS), pack_upsample_weight(wi, u, tdt).to(DEV)
    H.check(H.lib().dx_voc_upsample(H.ptr(xd), cin, H.ptr(wp), wdt, None, H.ptr(y), cout, H.ptr(nd), B, N, cin, cout, k, u, 1., H.stream()))
    assert torch.equal(y.double().cpu(), want)


@pytest.mark.parametrize('c', [32, 8])
def test_post_alone(c):
    from daft_exprt import _hip as H
    B, N, n = len(ROWS), max(ROWS), torch.tensor(ROWS)
    g = _gen(c)
    x = O.mask_rows(torch.randn((B, c, N), generator=g), n)
    w = torch.randn((1, c, 7), generator=g) * 0.3 / (c * 7) ** 0.5
    bias = 0.01 * torch.randn((1,), generator=g)
    o64, o32 = (O.post(x.to(dt), w, bias, n).double() for dt in (torch.float64, torch.float32))
    y = torch.full((B, N + 5), float('nan'), device=DEV)
    xd, wp, bd, nd = _rows_major(x, n=ROWS), w[0].t().contiguous().to(DEV), bias.to(DEV), n.to(DEV)
    H.check(H.lib().dx_voc_post(H.ptr(xd), c, H.ptr(wp), H.ptr(bd), H.ptr(y), N + 5, H.ptr(nd), B, N, c, 7, 0.01, H.stream()))
    assert bool(torch.isnan(y[:, N:]).all())                                                   # nothing past N is written
    _bound(y[:, :N], o64, o32, None, 'fp32', f'post {c}')
    for b, rows in enumerate(ROWS):
        assert float(y[b, rows:N].abs().max() if rows < N else 0.) == 0.


# ---- the whole generator ----------------------------------------------------------------------------------------------------

CASES = {'small': (O.SMALL, (23, 9, 1)), 'small_resblock2': (dict(O.SMALL, resblock='2'), (23, 9, 1)), 'v1': (O.V1, (12, 5)),
         'narrow': (O.NARROW, (23, 9, 1))}


@functools.lru_cache(maxsize=None)
def _case(name):
    ''' (cfg, lengths, mel with random values past the lengths, weights, oracle64, oracle32, oracle_rounded), computed once '''
    cfg, lengths = CASES[name]
    mel = O.make_mel(cfg, lengths, seed=3)
    weights = O.make_weights(cfg, mel, lengths, seed=3)
    n = torch.tensor(lengths)
    o64, o32, orr = _three(lambda dt, rounding: O.generator(cfg, weights, mel, n, rounding=rounding, dtype=dt).double())
    return cfg, lengths, mel, weights, o64, o32, orr


@functools.lru_cache(maxsize=None)
def _vocoder(name, dtype):
    from daft_exprt.vocoder import Vocoder
    cfg, _, _, weights, _, _, _ = _case(name)
    return Vocoder(cfg, O.state_dict(weights), compute_dtype=dtype, device=DEV)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(CASES))
def test_generator_matches_the_oracle(name, dtype):
    cfg, lengths, mel, _, o64, o32, orr = _case(name)
    hop = cfg['hop_size']
    assert float((o64.abs() > 0.95).double().mean()) < 0.01                                     # tanh saturation cannot hide an error
    wavs, n_samples = _vocoder(name, dtype)(mel.to(DEV), torch.tensor(lengths, device=DEV))
    assert wavs.shape == (len(lengths), max(lengths) * hop) and wavs.dtype == torch.float32
    assert n_samples.tolist() == [t * hop for t in lengths]
    _bound(wavs, o64, o32, orr, dtype, f'generator {name}')
    for b, t in enumerate(lengths):
        assert float(wavs[b, t * hop:].abs().max() if t < max(lengths) else 0.) == 0.
    assert float(wavs.abs().max()) <= 1.


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['small', 'v1', 'narrow'])
def test_batch_independence_bit_for_bit(name, dtype):
    cfg, lengths, mel, _, _, _, _ = _case(name)
    hop, voc = cfg['hop_size'], _vocoder(name, dtype)
    mel_d, n = mel.to(DEV), torch.tensor(lengths, device=DEV)
    wavs, _ = voc(mel_d, n)
    again, _ = voc(mel_d, n)
    assert torch.equal(wavs, again)                                                             # run to run
    split, _ = voc(mel_d, n, max_workspace_bytes=1)                                             # one utterance per sub-batch
    assert torch.equal(wavs, split)
    for b, t in enumerate(lengths):
        alone, n_alone = voc(mel_d[b:b + 1, :, :t].contiguous(), n[b:b + 1])
        assert alone.shape == (1, t * hop) and int(n_alone[0]) == t * hop
        assert torch.equal(alone[0], wavs[b, :t * hop]), (b, float((alone[0] - wavs[b, :t * hop]).abs().max()))
    order = list(reversed(range(len(lengths))))                                                  # another neighbour, another padded length
    swapped, _ = voc(torch.cat([mel_d[order], mel_d[order]], dim=2), n[order])
    for row, b in enumerate(order):
        assert torch.equal(swapped[row, :lengths[b] * hop], wavs[b, :lengths[b] * hop])


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['small', 'narrow'])
def test_nothing_past_the_end_is_read(name, dtype):
    from daft_exprt import config
    cfg, lengths, mel, _, _, _, _ = _case(name)
    voc = _vocoder(name, dtype)
    n = torch.tensor(lengths, device=DEV)
    clean, _ = voc(mel.to(DEV), n)
    dirty = mel.clone()
    for b, t in enumerate(lengths):
        dirty[b, :, t:] = float('nan')
    old = config.POISON
    config.POISON = True
    try:
        voc._ws = None                                                                          # a fresh, NaN-filled workspace
        got, _ = voc(dirty.to(DEV), n)
        torch.cuda.synchronize()
    finally:
        config.POISON = old
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, clean)


# ---- the public surface -----------------------------------------------------------------------------------------------------

SURFACE = {'resblock': '1', 'upsample_rates': [8, 8, 4], 'upsample_kernel_sizes': [16, 16, 8], 'upsample_initial_channel': 256,
           'resblock_kernel_sizes': [3], 'resblock_dilation_sizes': [[1, 3]], 'num_mels': 80, 'hop_size': 256, 'sampling_rate': 22050}


def _surface_weights():
    lengths = (4,)
    mel = O.make_mel(SURFACE, lengths, seed=7)
    return O.make_weights(SURFACE, mel, lengths, seed=7)


def _read_pcm16(path):
    raw = open(path, 'rb').read()
    assert raw[:4] == b'RIFF' and raw[8:12] == b'WAVE' and int.from_bytes(raw[20:22], 'little') == 1     # PCM
    assert int.from_bytes(raw[34:36], 'little') == 16 and int.from_bytes(raw[22:24], 'little') == 1      # 16 bits, mono
    return np.frombuffer(raw[raw.index(b'data') + 8:], dtype='<i2')


def test_generate_mel_specs_with_a_vocoder(golden_dir, tmp_path):
    from daft_exprt import generate as G
    from daft_exprt.vocoder import Vocoder, pcm16
    from tests.test_gpu_prosody_eval import SENTENCES, _style_bank, _tiny_model
    model, hp = _tiny_model(golden_dir)
    model = model.cuda(0)
    voc = Vocoder(SURFACE, O.state_dict(_surface_weights(), 'weight_norm'), compute_dtype='fp32', device=DEV)
    bank = str(tmp_path / 'bank')
    G.extract_reference_parameters_batch(_style_bank(bank, hp), bank, hp)
    refs = [os.path.join(bank, n) for n in ('glide.npz', 'vibrato.npz', 'glide.npz')]
    spk, names = [0, 3, 7], ['a', 'b', 'c']
    with pytest.raises(ValueError, match='use_griffin_lim'):
        G.generate_mel_specs(model, SENTENCES, list(names), spk, refs, str(tmp_path / 'none'), hp, scores={})
    scores = {}
    out_dir, plain_dir, again_dir = (str(tmp_path / d) for d in ('voc', 'plain', 'again'))
    preds = G.generate_mel_specs(model, SENTENCES, list(names), spk, refs, out_dir, hp, batch_size=3, scores=scores, vocoder=voc)
    plain = G.generate_mel_specs(model, SENTENCES, list(names), spk, refs, plain_dir, hp, batch_size=3)
    again = G.generate_mel_specs(model, SENTENCES, list(names), spk, refs, again_dir, hp, batch_size=3, vocoder=None)
    assert list(preds) == list(plain) == list(again) == list(scores) and len(preds) == 3
    assert sorted(os.listdir(plain_dir)) == sorted(os.listdir(again_dir)) == sorted(f'{name}.npz' for name in preds)
    assert sorted(os.listdir(out_dir)) == sorted([f'{name}.npz' for name in preds] + [f'{name}.wav' for name in preds])
    for name in preds:
        for other_dir, other in ((plain_dir, plain), (again_dir, again)):                       # the vocoder changes no other output
            assert open(os.path.join(out_dir, f'{name}.npz'), 'rb').read() == open(os.path.join(other_dir, f'{name}.npz'), 'rb').read()
            assert all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(preds[name], other[name]))
        mel = torch.from_numpy(preds[name][4]).to(DEV)[None]
        t = mel.shape[2]
        wav, n = voc(mel, torch.tensor([t], device=DEV))
        pcm = _read_pcm16(os.path.join(out_dir, f'{name}.wav'))
        assert pcm.shape == (t * hp.hop_length,) and int(n[0]) == t * hp.hop_length
        assert np.array_equal(pcm, pcm16(wav)[0].cpu().numpy())
        assert np.abs(pcm).max() > 100                                                          # audio, not silence
        got = scores[name]
        assert list(got) == ['pitch_pcc', 'energy_pcc', 'voiced_ref', 'voiced_gen', 'frames_ref', 'frames_gen']
        assert got['frames_gen'] == t + 1 and got['frames_ref'] > 40
        print(f'{name}: {got}')
    half = dict(SURFACE, upsample_rates=[8, 8, 2], upsample_kernel_sizes=[16, 16, 4], hop_size=128)
    bad = Vocoder(half, O.state_dict(O.make_weights(half, O.make_mel(half, (4,), seed=7), (4,), seed=7)), compute_dtype='fp32', device=DEV)
    with pytest.raises(ValueError, match='hop_length'):                                         # a vocoder of another front-end
        G.generate_mel_specs(model, SENTENCES, list(names), spk, refs, out_dir, hp, batch_size=3, vocoder=bad)


def test_synthesize_cli_with_a_vocoder(golden_dir, tmp_path):
    from tests.test_gpu_prosody_eval import _style_bank, _tiny_model
    model, hp = _tiny_model(golden_dir)
    ckpt = str(tmp_path / 'DaftExprt_test')
    torch.save({'iteration': 0, 'state_dict': dict(model.state_dict()), 'config_params': dict(vars(hp))}, ckpt)
    voc_dir = tmp_path / 'hifigan'
    voc_dir.mkdir()
    torch.save({'generator': O.state_dict(_surface_weights(), 'parametrizations')}, str(voc_dir / 'g_00000001'))
    (voc_dir / 'config.json').write_text(json.dumps(SURFACE))
    bank, out_dir = str(tmp_path / 'bank'), str(tmp_path / 'out')
    _style_bank(bank, hp)
    text = tmp_path / 'sentences_to_generate.txt'
    text.write_text('s.txt_line0|{HH AH0 L OW1} {W ER1 L D} , {T EH1 S T} ? ~\ns.txt_line1|{T EH1 S T} . ~\n', encoding='utf-8')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'synthesize.py'), '-out', out_dir, '-chk', ckpt, '-tf', str(text),
                        '-sb', bank, '-bs', '2', '-rtf', '-voc', str(voc_dir / 'g_00000001')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    report = json.load(open(os.path.join(out_dir, 'prosody_transfer.json')))
    assert report['audio'] == 'hifi-gan' and len(report['files']) == 2
    assert 'DaftExprt + HiFi-GAN RTF' in r.stderr
    for name, entry in report['files'].items():
        pcm = _read_pcm16(os.path.join(out_dir, entry['wav']))
        frames = np.load(os.path.join(out_dir, f'{name}.npz'))['mel_spec'].shape[1]
        assert pcm.shape == (frames * hp.hop_length,)
