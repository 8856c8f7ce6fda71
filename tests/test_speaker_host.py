"""The host side of the speaker-identity score, without a GPU: tests/speaker_oracle.py's pooling is pinned against
torch float64 autograd of the plain masked-softmax statement, its trial histograms against a double loop over all pairs, and
`speaker.eer_from_counts` against two other statements of the equal error rate; the host logic of daft_exprt/speaker.py (the scalar
normalisation, the masks of the encoder, checkpoints, the speaker count) on CPU tensors; the limits and symbols of K32 through the ABI."""
import numpy as np
import pytest
import torch

from tests import speaker_oracle as O
from tests.test_gpu_g2p import EPS, _bound


# ---- the pooling oracle ------------------------------------------------------------------------------------------------------------------

def test_pool_oracle_against_torch_autograd():
    rng = np.random.RandomState(0)
    n_steps = np.array([0, 1, 2, 5, 9, 7], dtype=np.int64)
    B, T, C = len(n_steps), 9, 5
    h, a, g = rng.standard_normal((B, T, C)) * 2 + 1, rng.standard_normal((B, T)) * 2, rng.standard_normal((B, 2 * C))
    dirty_h, dirty_a = h.copy(), a.copy()
    for b, n in enumerate(n_steps):
        dirty_h[b, n:], dirty_a[b, n:] = np.nan, np.nan                       # the oracle reads nothing at or past n_steps
    out, stat = O.pool(dirty_h, dirty_a, n_steps)
    g_h, g_a = O.pool_grad(dirty_h, dirty_a, n_steps, g)
    th, ta = torch.tensor(h, requires_grad=True), torch.tensor(a, requires_grad=True)
    want = O.pool_torch(th, ta, torch.tensor(n_steps))
    (want * torch.tensor(g)).sum().backward()
    assert np.abs(out - want.detach().numpy()).max() < 1e-12 and not out[0].any()
    assert np.abs(g_h - th.grad.numpy()).max() < 1e-12 and np.abs(g_a - ta.grad.numpy()).max() < 1e-12
    for b, n in enumerate(n_steps):
        assert not g_h[b, n:].any() and not g_a[b, n:].any()
        if n:
            assert stat[b, 0] == a[b, :n].max() and abs(stat[b, 1] - np.exp(a[b, :n] - a[b, :n].max()).sum()) < 1e-12
    assert np.abs(out[1, :C] - h[1, 0]).max() < 1e-12 and np.abs(out[1, C:] - np.sqrt(O.VAR_EPS)).max() < 1e-12   # one step: sd = sqrt(eps)
    lo, _ = O.pool(h.astype(np.float32), a.astype(np.float32), n_steps, np.float32)
    assert lo.dtype == np.float32 and np.abs(lo - out).max() < 1e-4


def test_the_one_pass_variance_misses_the_bound_the_two_pass_sets():
    ''' channels of mean 100 and deviation 0.1: the float32 restatement of sum w h^2 - mu^2 misses the GPU test's bound for that
        row -- max(4 x the float32 two-pass restatement's deviation from float64, 8 eps32 x the largest |h|) -- by orders '''
    c = O.offset_case()
    hi, _ = O.pool(c['h'], c['a'], c['n_steps'], np.float64)
    lo, _ = O.pool(c['h'], c['a'], c['n_steps'], np.float32)
    bound = _bound(hi, lo, float(np.abs(c['h']).max()))
    one_pass = np.abs(O.pool_one_pass(c['h'], c['a'], c['n_steps'], np.float32).astype(np.float64) - hi).max()
    two_pass = np.abs(lo.astype(np.float64) - hi).max()
    print(f'bound {bound:.3e}; float32 two-pass {two_pass:.3e}, float32 one-pass {one_pass:.3e}')
    assert abs(hi[0, c['C']:].mean() - 0.1) < 0.01 and abs(hi[0, :c['C']].mean() - 100) < 0.1
    assert two_pass <= bound < 1e-3 and one_pass > 10 * bound
    assert np.abs(O.pool_one_pass(c['h'], c['a'], c['n_steps'], np.float64) - hi).max() < 1e-6      # in float64 the shortcut is the same number


# ---- the trial oracle and the equal error rate -------------------------------------------------------------------------------------------

def test_trial_oracle_against_a_double_loop():
    rng = np.random.RandomState(1)
    for N, D, S in ((1, 3, 1), (2, 4, 1), (7, 5, 2), (12, 9, 3)):
        E = rng.standard_normal((N, D))
        E /= np.linalg.norm(E, axis=1, keepdims=True)
        spk = rng.randint(0, S, size=N)
        got = O.trial_counts(E, spk)
        assert got.shape == (2, O.BINS) and got.sum() == N * (N - 1) // 2 and np.array_equal(got, O.trial_counts_loops(E, spk))
    E, spk = O.exact_rows(12, 20, 2)
    got = O.trial_counts(E, spk)
    assert np.array_equal(got, O.trial_counts_loops(E, spk)) and got[:, O.BINS - 1].sum() >= 1 and got[:, 0].sum() >= 1   # s = 1 and s = -1
    assert np.allclose(np.linalg.norm(O.exact_rows(30, 200, 3)[0], axis=1), 1.0, atol=0, rtol=0)
    assert not O.trial_counts(E, np.zeros(12, dtype=np.int32))[1].any()      # one speaker: no non-target trial


def test_eer_from_counts_against_sorted_scores():
    from daft_exprt.speaker import eer_from_counts
    rng = np.random.RandomState(2)
    edges = np.arange(O.BINS + 1) / 2048.0 - 1.0
    for trial in range(6):
        n_tar, n_non = (40, 300) if trial < 3 else (500, 77)
        tar_bins = np.clip(np.round(rng.normal(2600, 120 + 60 * trial, n_tar)), 0, O.BINS - 1).astype(int)
        non_bins = np.clip(np.round(rng.normal(2300, 150, n_non)), 0, O.BINS - 1).astype(int)
        counts = np.stack([np.bincount(tar_bins, minlength=O.BINS), np.bincount(non_bins, minlength=O.BINS)])
        centre = lambda b: (b + 0.5) / 2048.0 - 1.0
        want_eer, want_th = O.eer_sorted(centre(tar_bins), centre(non_bins), edges)
        got = eer_from_counts(counts)
        assert got == (want_eer, want_th) and 0 < got[0] < 0.5                # exactly: the same fractions, the lowest threshold on a tie
        assert got[0] == O.eer_loop(counts)[0] and got[1] == O.eer_loop(counts)[1] / 2048.0 - 1.0
        assert eer_from_counts(torch.tensor(counts)) == got


def test_eer_from_counts_degenerate():
    from daft_exprt.speaker import eer_from_counts
    z = np.zeros((2, O.BINS), dtype=np.int64)
    only_tar, only_non = z.copy(), z.copy()
    only_tar[0, 3000], only_non[1, 2000] = 5, 5
    assert eer_from_counts(z) is None and eer_from_counts(only_tar) is None and eer_from_counts(only_non) is None
    apart = z.copy()
    apart[0, 3000:3010], apart[1, 1990:2001] = 4, 9
    assert eer_from_counts(apart) == (0.0, 2001 / 2048.0 - 1.0)              # the lowest threshold that accepts no non-target
    same = z.copy()
    same[:, 2040:2050] = 3
    eer, th = eer_from_counts(same)
    assert eer == 0.5 and th == 2045 / 2048.0 - 1.0                          # FAR + FRR = 1 at every threshold; equal in the middle
    flipped = z.copy()
    flipped[0, 1000], flipped[1, 3000] = 7, 7                                # every target below every non-target
    assert eer_from_counts(flipped)[0] >= 0.5
    assert eer_from_counts(apart) == O.eer_loop(apart)[:1] + (O.eer_loop(apart)[1] / 2048.0 - 1.0,)


# ---- the host logic of the model ---------------------------------------------------------------------------------------------------------

def _oracle_embed(enc, mel, n):
    ''' the encoder with the pooling replaced by its float64 oracle on the CPU '''
    h, a, n_steps = enc.frames(mel, n)
    pooled, _ = O.pool(h.double().numpy(), a.double().numpy(), n_steps.numpy())
    return enc.out(torch.tensor(pooled, dtype=torch.float32)), h, a, n_steps


def test_the_scalar_normalisation_ignores_what_lies_past_n_frames():
    from daft_exprt.speaker import SpeakerEncoder
    torch.manual_seed(0)
    enc = SpeakerEncoder(6, hidden=8, layers=1)
    n = torch.tensor([13, 8, 1, 0])
    mel = torch.randn(4, 6, 13) * 3.0 - 5.0 + torch.randn(1, 6, 1)
    dirty = mel.clone()
    for b in range(4):
        dirty[b, :, int(n[b]):] = float('nan') if b % 2 else 1e4
    x = enc.normalise(dirty, n)
    assert x.shape == (4, 13, 6) and torch.isfinite(x).all()
    for b in range(4):
        live = x[b, :int(n[b])]
        assert not x[b, int(n[b]):].any()
        if int(n[b]):
            assert abs(float(live.mean())) < 1e-5 and abs(float((live * live).mean()) - 1) < 1e-3    # ONE mean and variance per utterance
            assert torch.equal(live, enc.normalise(mel[b:b + 1, :, :int(n[b])].contiguous(), n[b:b + 1])[0])
    # the spectral shape survives: the channel means keep their differences (a per-channel normalisation would zero them)
    assert float(x[0, :13].mean(0).std()) > 0.05
    shifted = enc.normalise(mel[:1] * 2.0 + 7.0, n[:1])                      # level and gain do not
    assert torch.allclose(shifted, x[:1], atol=1e-4)


@pytest.mark.parametrize('stride', (1, 2, 3))
def test_forward_batched_equals_alone(stride):
    from daft_exprt.speaker import SpeakerEncoder
    torch.manual_seed(0)
    enc = SpeakerEncoder(6, hidden=16, layers=3, stride=stride, dim=8).eval()
    n = torch.tensor([13, 8, 1, 7])
    mel = torch.randn(4, 6, 13) * 3.0 - 5.0
    dirty = mel.clone()
    for b in range(4):
        dirty[b, :, int(n[b]):] = float('nan') if b % 2 else 1e4
    with torch.no_grad():
        emb, h, a, n_steps = _oracle_embed(enc, dirty, n)
        assert n_steps.tolist() == [-(-int(v) // stride) for v in n] == enc.n_steps_of(n).tolist()
        assert h.shape == (4, -(-13 // stride), 16) and a.shape == h.shape[:2] and h.is_contiguous() and a.is_contiguous()
        assert emb.shape == (4, 8) and torch.isfinite(emb).all()
        for b in range(4):
            alone, _, _, steps = _oracle_embed(enc, mel[b:b + 1, :, :int(n[b])].contiguous(), n[b:b + 1])
            assert int(steps) == int(n_steps[b])
            assert torch.allclose(emb[b], alone[0], rtol=1e-4, atol=1e-5), b


def test_am_softmax_and_centroids():
    from daft_exprt.speaker import am_softmax_loss, speaker_centroids
    torch.manual_seed(1)
    e, w, t = torch.randn(5, 4), torch.randn(3, 4), torch.tensor([0, 2, 1, 1, 0])
    cos = torch.nn.functional.normalize(e, dim=1) @ torch.nn.functional.normalize(w, dim=1).t()
    logits = 30.0 * cos
    logits[torch.arange(5), t] -= 30.0 * 0.2
    assert torch.allclose(am_softmax_loss(e, w, t), torch.nn.functional.cross_entropy(logits, t))
    assert torch.allclose(am_softmax_loss(7 * e, 3 * w, t), am_softmax_loss(e, w, t), atol=1e-5)          # lengths do not matter
    unit = torch.nn.functional.normalize(e, dim=1)
    c = speaker_centroids(unit, t, 4)
    assert c.shape == (4, 4) and torch.allclose(c[:3].norm(dim=1), torch.ones(3)) and not c[3].any()
    assert torch.allclose(c[1], torch.nn.functional.normalize(unit[2] + unit[3], dim=0))


def test_save_load_round_trip(tmp_path):
    from daft_exprt.speaker import SpeakerEncoder, load_speaker_encoder, save_speaker_encoder
    torch.manual_seed(2)
    enc = SpeakerEncoder(6, hidden=8, layers=2, stride=3, dim=5).eval()
    centroids = torch.nn.functional.normalize(torch.randn(3, 5), dim=1)
    enc.set_speakers([4, 9, 11], centroids, threshold=0.25, eer=0.0625)
    path = str(tmp_path / 'speaker.pt')
    save_speaker_encoder(enc, path)
    back = load_speaker_encoder(path, device='cpu')
    assert back.args == enc.args == dict(n_mel=6, hidden=8, layers=2, stride=3, dim=5) and not back.training
    assert back.speaker_ids == [4, 9, 11] and torch.equal(back.centroids, centroids) and (back.threshold, back.eer) == (0.25, 0.0625)
    assert 'centroids' not in enc.state_dict() and set(back.state_dict()) == set(enc.state_dict())
    for k, v in enc.state_dict().items():
        assert torch.equal(back.state_dict()[k], v)
    mel, n = torch.randn(2, 6, 10), torch.tensor([10, 4])
    with torch.no_grad():
        assert torch.equal(_oracle_embed(back, mel, n)[0], _oracle_embed(enc, mel, n)[0])


def test_training_refuses_one_speaker(tmp_path):
    from daft_exprt.speaker import list_speakers, train_speaker_encoder
    one = tmp_path / 'one.txt'
    one.write_text('/nowhere|a|3\n/nowhere|b|3\n\n', encoding='utf-8')
    assert list_speakers(str(one)) == [3, 3]
    with pytest.raises(ValueError, match='at least 2'):
        train_speaker_encoder(None, str(one), None)


def test_the_wrappers_need_a_gpu():
    from daft_exprt.speaker import SpeakerEncoder, attn_stat_pool, speaker_scores, trial_counts
    with pytest.raises(RuntimeError, match='device tensors'):                # no CPU fallback
        attn_stat_pool(torch.zeros(1, 2, 3), torch.zeros(1, 2), torch.tensor([2]))
    with pytest.raises(RuntimeError, match='device tensors'):
        trial_counts(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int32))
    enc = SpeakerEncoder(4, hidden=8, layers=1, dim=3)
    with pytest.raises(RuntimeError, match='device tensors'):
        enc.embed(torch.zeros(1, 4, 6), torch.tensor([6]))
    enc.set_speakers([0, 1], torch.eye(2, 3))
    with pytest.raises(RuntimeError, match='device tensors'):
        speaker_scores(enc, torch.zeros(1, 4, 6), torch.tensor([6]), [0])


def test_toy_corpus_and_ceilings():
    train, held = O.toy_corpus()
    T = O.TOY
    assert len(train) == 6 * 30 and len(held) == 6 * 10 and [u[0] for u in held] == [s for s in range(6) for _ in range(10)]
    assert all(u[1].shape[1] == T['n_mel'] and 8 <= u[1].shape[0] <= 84 for u in train + held)
    offsets = O.toy_offsets()
    assert offsets.shape == (6, 16) and float(offsets.std()) > 0.5 * T['offset']
    mel, n, spk = O.toy_collate(held[:3], torch.float64)
    assert mel.shape[:2] == (3, 16) and int(n.max()) == mel.shape[2] and spk.tolist() == [0, 0, 0]
    assert len(O.toy_batches(0, 180)) == T['steps'] and all(len(b) == T['batch'] for b in O.toy_batches(0, 180)[:3])
    assert len(O.RESTATEMENT_ID) == len(O.RESTATEMENT_EER) == 6
    assert O.CEILING_ID == 2 * max(O.RESTATEMENT_ID) - min(O.RESTATEMENT_ID) < 0.2
    assert O.CEILING_EER == 2 * max(O.RESTATEMENT_EER) - min(O.RESTATEMENT_EER) < 0.2


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------

def test_limits_and_symbols_through_the_abi():
    from daft_exprt import _hip as H
    from daft_exprt.speaker import limits
    lib = H.lib()
    assert lib.dx_abi_version() == 13
    assert limits() == (lib.dx_spk_pool_max_channels(), lib.dx_spk_pool_max_steps(), lib.dx_trial_max_dim(), lib.dx_trial_max_rows())
    assert limits() == (1024, 4096, 1024, 65536)
    declared = {name for name, _, _ in H.header_prototypes()}
    assert {'dx_spk_pool_max_channels', 'dx_spk_pool_max_steps', 'dx_trial_max_dim', 'dx_trial_max_rows', 'dx_attn_stat_pool_fwd',
            'dx_attn_stat_pool_bwd', 'dx_trial_counts'} <= declared
    for T, C in ((4097, 8), (8, 1025)):                                      # beyond a limit: a code and a message before any launch
        assert lib.dx_attn_stat_pool_fwd(8, 8, 8, 8, 8, 1, T, C, None) == -5 and b'at most' in lib.dx_last_error()
        assert lib.dx_attn_stat_pool_bwd(8, 8, 8, 8, 8, 8, 8, 8, 8, 1, T, C, None) == -5 and b'at most' in lib.dx_last_error()
    assert lib.dx_attn_stat_pool_fwd(8, 8, 8, 8, 8, 0, 4, 4, None) == -2 and lib.dx_attn_stat_pool_fwd(8, 8, 8, 8, 8, 1, 4, 0, None) == -2
    assert lib.dx_trial_counts(8, 8, 8, 65537, 4, None) == -5 and b'at most' in lib.dx_last_error()
    assert lib.dx_trial_counts(8, 8, 8, 4, 1025, None) == -5 and lib.dx_trial_counts(8, 8, 8, 0, 4, None) == -2
    assert lib.dx_attn_stat_pool_fwd(None, 8, 8, 8, 8, 1, 4, 4, None) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_attn_stat_pool_bwd(8, 8, 8, 8, 8, 8, 8, 8, None, 1, 4, 4, None) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_trial_counts(8, None, 8, 4, 4, None) == -1 and lib.dx_trial_counts(8, 8, None, 4, 4, None) == -1
