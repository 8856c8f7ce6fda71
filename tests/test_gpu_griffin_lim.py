"""Griffin-Lim preview path on the GPU (`daft_exprt/griffin_lim.py`, csrc/griffin_lim.hip) against the reference's
`griffin_lim.py` as recorded in tests/golden/griffin_lim.npz and against its float64 restatement
(tests/griffin_lim_oracle.py).

Tolerances: NNLS -- the reference stops L-BFGS-B early and x is not unique, so the contract is the objective: per frame
|| A x - b || / || b || <= reference * (1 + 1e-3) + 1e-4.  Griffin-Lim from the reference's own start signal (float32 of
the seeded np.random.randn): 1e-5 relative L2 after 1 iteration, 1e-3 after 30, 2e-3 max |diff| of the normalised signal
(fp32 FFTs against float64: ~1e-6 / 1e-5 / 1e-4 in a float32 NumPy restatement, so 10-100x headroom)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import griffin_lim_oracle as O
from tests.util import make_hparams

DEV = torch.device('cuda:0')
GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'griffin_lim.npz')


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _lin(mags, T):
    ''' list of (n_fft/2 + 1, T_b) magnitudes -> (B, n_fft/2 + 1, T) zero-padded device tensor + lengths '''
    out = torch.zeros((len(mags), mags[0].shape[0], T), dtype=torch.float32)
    for b, m in enumerate(mags):
        out[b, :, :m.shape[1]] = torch.as_tensor(np.asarray(m, dtype=np.float32))
    return out.to(DEV), torch.tensor([m.shape[1] for m in mags], dtype=torch.int64, device=DEV)


def test_mel_to_linear_objective_at_least_as_good_as_reference():
    from daft_exprt import griffin_lim as G
    fx = np.load(GOLD)
    hp = make_hparams()
    A = O.filterbank(hp)
    for name in ('dec', 'cone', 'noisy', 'edge'):
        mel = fx[f'nnls_{name}_mel']
        n_mel, T = mel.shape
        batch = torch.zeros((2, n_mel, T + 5), dtype=torch.float32)
        batch[0, :, :T] = torch.as_tensor(mel)
        batch[1, :, :T] = torch.as_tensor(mel)
        lengths = torch.tensor([T, T - 1], dtype=torch.int64, device=DEV)
        lin = G.mel_to_linear_batch(batch.to(DEV), lengths, hp).cpu().numpy()
        assert lin.shape == (2, hp.filter_length // 2 + 1, T + 5)
        assert np.isfinite(lin).all() and (lin >= 0).all()
        assert (lin[0, :, T:] == 0).all() and (lin[1, :, T - 1:] == 0).all()           # frames past lengths
        b = np.exp(mel)
        res = O.rel_residual(A, lin[0, :, :T], b)
        ref = fx[f'nnls_{name}_relres']
        assert (res <= ref * (1 + 1e-3) + 1e-4).all(), (name, np.max(res - ref), np.argmax(res - ref))
        assert np.array_equal(lin[1, :, :T - 1], lin[0, :, :T - 1])                      # frames are independent
        lin1 = G.mel_to_linear(b, hp)                                                    # reference signature: linear mel in
        assert lin1.shape == (hp.filter_length // 2 + 1, T)
        assert (O.rel_residual(A, lin1, b) <= ref * (1 + 1e-3) + 1e-4).all()


@pytest.mark.parametrize('T', [3, 24, 64, 100])
def test_griffin_lim_matches_reference_from_its_start_signal(T):
    from daft_exprt import griffin_lim as G
    fx = np.load(GOLD)
    hp = make_hparams()
    S = O.n_samples(T, hp.filter_length, hp.hop_length)
    x0 = torch.as_tensor(O.reference_start(int(fx[f'gl_{T}_seed']), S).astype(np.float32)).reshape(1, S).to(DEV)
    lin, lengths = _lin([O.harmonic_magnitude(T)], T)
    w1, n1 = G.griffin_lim_from_linear(lin, lengths, hp, iterations=1, x0=x0, normalise=False)
    w30, _ = G.griffin_lim_from_linear(lin, lengths, hp, iterations=30, x0=x0, normalise=False)
    wn, _ = G.griffin_lim_from_linear(lin, lengths, hp, iterations=30, x0=x0)
    assert int(n1[0]) == S and w1.shape == (1, S)
    want1 = fx[f'gl_{T}_sig1'] if f'gl_{T}_sig1' in fx.files else \
        O.griffin_lim(O.harmonic_magnitude(T)[:, :-2], hp.hop_length, 1, x0[0].double().cpu().numpy())[0][0]
    assert _rel(w1[0].cpu().numpy(), want1) <= 1e-5
    sig30 = fx[f'gl_{T}_sig30']
    assert _rel(w30[0].cpu().numpy(), sig30) <= 1e-3
    assert np.abs(wn[0].cpu().numpy() - sig30 / np.abs(sig30).max()).max() <= 2e-3
    assert float(wn.abs().max()) == 1.
    sig, proposal = G.reconstruct_signal_griffin_lim(O.harmonic_magnitude(T)[:, :-2], hp.hop_length, 30, None,
                                                     x0=x0[0].cpu().numpy())
    assert sig.dtype == np.float64 and np.array_equal(sig, w30[0].double().cpu().numpy())
    assert proposal.shape == (T - 2, hp.filter_length // 2 + 1)


def test_ragged_batch_equals_each_utterance_alone():
    from daft_exprt import griffin_lim as G
    hp = make_hparams()
    n_fft, hop = hp.filter_length, hp.hop_length
    Ts = [100, 3, 64, 2, 24, 1]
    Tm = max(Ts)
    mags = [O.harmonic_magnitude(T, f0=110. + 7 * i) for i, T in enumerate(Ts)]
    lin, lengths = _lin(mags, Tm)
    rng = np.random.RandomState(5)
    x0s = [rng.randn(O.n_samples(T, n_fft, hop)).astype(np.float32) for T in Ts]
    X0 = torch.zeros((len(Ts), O.n_samples(Tm, n_fft, hop)), dtype=torch.float32)
    for b, x in enumerate(x0s):
        X0[b, :len(x)] = torch.as_tensor(x)
    for normalise in (False, True):
        wav, n = G.griffin_lim_from_linear(lin, lengths, hp, iterations=5, x0=X0.to(DEV), normalise=normalise)
        wav, n = wav.cpu(), n.cpu()
        assert torch.isfinite(wav).all()
        for b, T in enumerate(Ts):
            S = O.n_samples(T, n_fft, hop)
            assert int(n[b]) == S == max(T - 2, 0) * hop + n_fft
            l1, len1 = _lin([mags[b]], T)
            w1, n1 = G.griffin_lim_from_linear(l1, len1, hp, iterations=5, x0=torch.as_tensor(x0s[b]).reshape(1, -1).to(DEV),
                                               normalise=normalise)
            assert int(n1[0]) == S and w1.shape[1] == S
            assert torch.equal(wav[b, :S], w1[0].cpu()), (T, normalise)
            assert (wav[b, S:] == 0).all()
            if T <= 2:
                assert (wav[b] == 0).all()                     # no frame: zeros, not the reference's 0 / 0


def test_seeded_device_noise():
    from daft_exprt import griffin_lim as G
    hp = make_hparams()
    lengths = torch.tensor([1000, 1000, 1000, 1000, 500], dtype=torch.int64, device=DEV)
    a, b, c = (G.device_noise(lengths, hp, 1000, seed=s) for s in (11, 11, 12))
    assert torch.equal(a, b) and not torch.equal(a, c)
    S5 = O.n_samples(500, hp.filter_length, hp.hop_length)
    assert (a[4, S5:] == 0).all()
    v = a[:4].double()
    assert v.numel() >= 10 ** 6
    assert abs(float(v.mean())) < 0.01 and abs(float(v.std()) - 1.) < 0.01
    assert abs(float((v > 0).double().mean()) - 0.5) < 0.01
    mel = torch.randn((2, hp.n_mel_channels, 60), generator=torch.Generator().manual_seed(3)).to(DEV) - 3.
    L = torch.tensor([60, 41], dtype=torch.int64, device=DEV)
    w1, _ = G.griffin_lim_batch(mel, L, hp, iterations=4, seed=7, nnls_iters=50)
    w2, _ = G.griffin_lim_batch(mel, L, hp, iterations=4, seed=7, nnls_iters=50)
    w3, _ = G.griffin_lim_batch(mel, L, hp, iterations=4, seed=8, nnls_iters=50)
    assert torch.equal(w1, w2) and not torch.equal(w1, w3)


def test_at_size_monotone_and_matches_oracle():
    ''' configs[3]-shaped batch: B = 256 utterances the synthesis pass generated (lengths up to ~1000 frames) '''
    import bench
    from daft_exprt import griffin_lim as G
    from daft_exprt.data_loader import centre_duration_head, synthetic_inference_batch
    from daft_exprt.model import DaftExprt
    hp = bench.make_hparams(256, 'bf16')
    hp.stats = {f'spk {i}': {'pitch': {'mean': 5.0, 'std': 0.3}} for i in range(hp.n_speakers)}
    torch.manual_seed(hp.seed)
    model = DaftExprt(hp).to(DEV).eval()
    centre_duration_head(model)
    with torch.no_grad():
        _, (mel, lengths), _ = model.inference(tuple(t.to(DEV) for t in synthetic_inference_batch(hp, 256, seed=1234)), 'add', hp)
    mel = mel.float().contiguous()
    B, _, T = mel.shape
    n_fft, hop = hp.filter_length, hp.hop_length
    lin = G.mel_to_linear_batch(mel, lengths, hp)
    x0 = G.device_noise(lengths, hp, T, seed=3)
    F = (lengths - 2).clamp(min=0)
    window = torch.as_tensor(np.hanning(n_fft), dtype=torch.float32, device=DEV)
    fmask = (torch.arange(T - 2, device=DEV)[None, :] < F[:, None]).float()[:, :, None]

    def inconsistency(x):
        frames = x.unfold(1, n_fft, hop)[:, :T - 2] * window
        spec = torch.fft.rfft(frames, dim=2).abs()
        d = (spec - lin[:, :, :T - 2].transpose(1, 2)) * fmask
        return d.double().pow(2).sum((1, 2)).sqrt()

    prev = None
    for k in range(1, 7):
        x, n = G.griffin_lim_from_linear(lin, lengths, hp, iterations=k, x0=x0, normalise=False)
        inc = inconsistency(x)
        assert torch.isfinite(inc).all()
        if prev is not None:
            assert (inc <= prev * (1 + 1e-5)).all(), (k, float((inc / prev).max()))
        prev = inc
    assert torch.equal(n, F * hop + n_fft)
    x30, _ = G.griffin_lim_from_linear(lin, lengths, hp, iterations=30, x0=x0, normalise=False)
    for b in (0, 85, 170, 255):
        Fb, Sb = int(F[b]), int(n[b])
        want = O.griffin_lim(lin[b, :, :Fb].double().cpu().numpy(), hop, 30, x0[b, :Sb].double().cpu().numpy())[0][-1]
        assert _rel(x30[b, :Sb].cpu().numpy(), want) <= 1e-3, b


def test_generate_writes_preview_wavs(golden_dir, tmp_path):
    import json
    from daft_exprt import generate as Gen
    from daft_exprt.model import DaftExprt
    from oracle import daft_exprt_cpu as OC
    from oracle.fill import fill_params
    from tests.util import load_driver_fixture
    st = np.load(os.path.join(golden_dir, 'inference.npz'))
    hp = make_hparams(compute_dtype='fp32')
    hp.stats = {f'spk {i}': {'pitch': {'mean': float(st['stats_pitch_mean'][i]), 'std': float(st['stats_pitch_std'][i])}}
                for i in range(11)}
    model = DaftExprt(hp)
    model.load_state_dict(fill_params(OC.param_shapes(hp)))
    model = model.cuda(0)
    ref_dir, out_dir = str(tmp_path / 'refs'), str(tmp_path / 'out')
    os.makedirs(ref_dir)
    sentences, dur_f, en_f, pi_f, refs, spk, names, fx = load_driver_fixture(golden_dir, 'add', ref_dir)
    preds = Gen.generate_mel_specs(model, sentences, list(names), spk, refs, out_dir, hp, dur_factors=dur_f, energy_factors=en_f,
                                   pitch_factors=['ADD', pi_f], batch_size=2, n_jobs=1, use_griffin_lim=True)
    npz = json.loads(str(fx['add_drv_files_json']))
    assert sorted(os.listdir(out_dir)) == sorted(npz + [f'{k}.wav' for k in preds])
    for key, vals in preds.items():
        assert np.array_equal(np.load(os.path.join(out_dir, f'{key}.npz'))['mel_spec'], vals[4])
        raw = open(os.path.join(out_dir, f'{key}.wav'), 'rb').read()
        i = raw.index(b'data')
        wav = np.frombuffer(raw[i + 8:], dtype='<f8')
        assert raw[20:22] == b'\x03\x00' and len(wav) == O.n_samples(vals[4].shape[1], hp.filter_length, hp.hop_length)
        assert np.isfinite(wav).all() and np.abs(wav).max() == 1.
        try:
            from scipy.io import wavfile
        except ImportError:
            continue
        sr, w2 = wavfile.read(os.path.join(out_dir, f'{key}.wav'))
        assert sr == hp.sampling_rate and np.array_equal(w2, wav)
