"""K32 (csrc/speaker.hip) and daft_exprt/speaker.py on the GPU against tests/speaker_oracle.py.

The pooling is compared with the float64 oracle on the same (fp32-representable) inputs under the project's measured bound, `_bound`
of tests/test_gpu_g2p.py, imported: 4 x the deviation of the float32 restatement from float64 on the same inputs, with a floor of
8 fp32 ulps of the scale -- the largest |h| of the row for `out`, the largest |g_out| x the largest |h| for the gradients.  The trial
histograms are integers: on rows whose dot products are exact in fp32 they must EQUAL the oracle's, and on random unit rows the
cumulative counts may differ by no more than the pairs whose float64 score lies within the fp32 error of a bin edge.  Every pooling
launch gets its dead inputs as NaN and its outputs and workspace pre-filled with NaN, and every row is run in the ragged batch, in a
batch with larger padded extents, and alone: the three must agree bit for bit."""
import functools
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import speaker_oracle as O
from tests.test_gpu_g2p import EPS, _bound, _close, _dev

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- dx_attn_stat_pool_fwd / dx_attn_stat_pool_bwd ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(C):
    ''' a ragged batch of `speaker_oracle.pool_case` (C = 0: the offset row), the float64 oracle and the float32 restatement, once '''
    c = O.pool_case(C) if C else O.offset_case()
    for tag, dt in (('hi', np.float64), ('lo', np.float32)):
        c['out_' + tag], c['stat_' + tag] = O.pool(c['h'], c['a'], c['n_steps'], dt)
        c['gh_' + tag], c['ga_' + tag] = O.pool_grad(c['h'], c['a'], c['n_steps'], c['g_out'], dt)
    return c


def _run(c, rows=None, pad=(0, 0)):
    ''' forward and backward on the rows `rows` of a case (all by default) with the tight extents plus `pad` = (T, B): h and a at or
        past n_steps NaN, the padded batch rows without steps; outputs and workspace poisoned '''
    from daft_exprt import _hip as H
    rows = list(range(c['B'])) if rows is None else rows
    n_steps = c['n_steps'][rows]
    B, C = len(rows) + pad[1], c['C']
    T = max(1, int(n_steps.max())) + pad[0]
    h, a = np.full((B, T, C), np.nan, dtype=np.float32), np.full((B, T), np.nan, dtype=np.float32)
    g_out, nT = np.full((B, 2 * C), 1.0, dtype=np.float32), np.zeros((B,), dtype=np.int64)
    for i, b in enumerate(rows):
        h[i, :n_steps[i]], a[i, :n_steps[i]], g_out[i], nT[i] = c['h'][b, :n_steps[i]], c['a'][b, :n_steps[i]], c['g_out'][b], n_steps[i]
    hd, ad, gd, nd = _dev(h), _dev(a), _dev(g_out), _dev(nT)
    nan = lambda *shape: torch.full(shape, float('nan'), device=DEV)
    o = dict(out=nan(B, 2 * C), stat=nan(B, 2), g_h=nan(B, T, C), g_a=nan(B, T))
    ws = nan(B, (C + 63) // 64, T)
    H.check(H.lib().dx_attn_stat_pool_fwd(H.ptr(hd), H.ptr(ad), H.ptr(nd), H.ptr(o['out']), H.ptr(o['stat']), B, T, C, H.stream()))
    H.check(H.lib().dx_attn_stat_pool_bwd(H.ptr(hd), H.ptr(ad), H.ptr(nd), H.ptr(o['out']), H.ptr(o['stat']), H.ptr(gd), H.ptr(o['g_h']),
                                          H.ptr(o['g_a']), H.ptr(ws), B, T, C, H.stream()))
    return {name: t.cpu().numpy() for name, t in o.items()}


def _row(out, i, n):
    ''' the bytes of row i of the outputs of `_run`, after checking that the gradients at or past n_steps are +0 '''
    for name in ('g_h', 'g_a'):
        dead = out[name][i, n:]
        assert not dead.any() and not np.signbit(dead).any(), name
    return out['out'][i].tobytes() + out['stat'][i].tobytes() + out['g_h'][i, :n].tobytes() + out['g_a'][i, :n].tobytes()


def _check_pool_case(c, tag):
    batch, again = _run(c), _run(c)
    for name in batch:                                                       # two runs: bit-equal
        assert batch[name].tobytes() == again[name].tobytes(), name
    wide = _run(c, pad=(5, 2))                                               # (T + 5, B + 2)
    for name in wide:
        assert not wide[name][c['B']:].any(), name                           # the rows without steps: zeros everywhere
    C = c['C']
    for b, n in enumerate(c['n_steps'].tolist()):
        alone = _run(c, rows=[b])
        assert _row(batch, b, n) == _row(alone, 0, n) == _row(wide, b, n), (tag, n)
        if n == 0:
            assert not batch['out'][b].any() and not batch['stat'][b].any()
            continue
        largest = float(np.abs(c['h'][b, :n]).max())
        g_scale = float(np.abs(c['g_out'][b]).max()) * largest
        _close(f'{tag} n={n} out', batch['out'][b], c['out_hi'][b], _bound(c['out_hi'][b], c['out_lo'][b], largest))
        _close(f'{tag} n={n} stat', batch['stat'][b], c['stat_hi'][b],
               _bound(c['stat_hi'][b], c['stat_lo'][b], max(float(np.abs(c['a'][b, :n]).max()), float(c['stat_hi'][b, 1]))))
        _close(f'{tag} n={n} g_h', batch['g_h'][b, :n], c['gh_hi'][b, :n], _bound(c['gh_hi'][b, :n], c['gh_lo'][b, :n], g_scale))
        _close(f'{tag} n={n} g_a', batch['g_a'][b, :n], c['ga_hi'][b, :n], _bound(c['ga_hi'][b, :n], c['ga_lo'][b, :n], g_scale))
        assert (batch['out'][b, C:] > 0).all()


@pytest.mark.parametrize('C', O.POOL_CHANNELS)
def test_pooling_against_float64_alone_in_a_batch_and_padded(C):
    ''' C = 20 (not a multiple of 8), 64, 192, 260 (four 64-channel blocks and a tail of 4) x rows of 0, 1, 2, 63, 64, 65, 255, 256,
        257 and 1000 steps in one batch.  The test prints every row's own error and bound. '''
    _check_pool_case(_case(C), f'C={C}')


def test_the_variance_is_taken_about_the_mean():
    ''' one row of 257 steps x 64 channels of mean 100 and deviation 0.1 under the bound its float32 TWO-pass restatement sets
        (tests/test_speaker_host.py shows that the one-pass sum w h^2 - mu^2 misses it by orders: 1e-1 against 2.5e-4) '''
    c = _case(0)
    _check_pool_case(c, 'offset row')
    out = _run(c)['out'][0]
    assert abs(float(out[c['C']:].mean()) - 0.1) < 0.01


def test_autograd_against_float64_in_a_small_graph():
    ''' relu(x W) -> (h, a = h v) -> attn_stat_pool -> Linear -> sum of squares: the gradients of x, W and v against float64 torch
        autograd of `speaker_oracle.pool_torch` on the CPU, under the bound the float32 CPU run of the same graph sets, with the
        scale |gradient into the pool| x |h| '''
    from daft_exprt.speaker import attn_stat_pool
    rng = np.random.RandomState(4)
    B, T, Cin, C = 5, 70, 12, 72
    n = torch.tensor([70, 1, 0, 33, 64])
    leaves = {k: torch.tensor(v, dtype=torch.float32) for k, v in
              (('x', rng.standard_normal((B, T, Cin))), ('W', rng.standard_normal((Cin, C)) / 3), ('v', rng.standard_normal((C,)) / 3),
               ('P', rng.standard_normal((2 * C, 6)) / 6))}

    def graph(pool, dtype, dev):
        t = {k: v.clone().to(dev, dtype).requires_grad_(k != 'P') for k, v in leaves.items()}
        live = (torch.arange(T, device=dev)[None] < n.to(dev)[:, None])[:, :, None]
        h = torch.where(live, torch.relu(t['x'] @ t['W']), torch.zeros((), dtype=dtype, device=dev))
        pooled = pool(h.contiguous(), (h @ t['v']).contiguous(), n.to(dev))
        pooled.retain_grad()
        ((pooled @ t['P']) ** 2).sum().backward()
        return {k: t[k].grad.cpu().double().numpy() for k in ('x', 'W', 'v')}, pooled.grad.abs().max().item(), h.abs().max().item(), pooled

    hi, g_max, h_max, pooled_hi = graph(O.pool_torch, torch.float64, 'cpu')
    lo, _, _, pooled_lo = graph(O.pool_torch, torch.float32, 'cpu')
    got, _, _, pooled = graph(attn_stat_pool, torch.float32, DEV)
    _close('pooled', pooled.detach().cpu().numpy(), pooled_hi.detach().numpy(), _bound(pooled_hi.detach().numpy(), pooled_lo.detach().numpy(), h_max))
    for k in ('x', 'W', 'v'):
        _close(f'grad {k}', got[k], hi[k], _bound(hi[k], lo[k], g_max * h_max))
    assert not got['x'][2].any() and not got['x'][1, 1:].any()              # nothing flows into dead steps


def test_pooling_argument_errors_are_codes():
    from daft_exprt import _hip as H
    from daft_exprt.speaker import attn_stat_pool, limits
    lib = H.lib()
    max_c, max_t, _, _ = limits()
    buf = torch.zeros(4096, device=DEV)
    n = torch.ones(4, dtype=torch.int64, device=DEV)
    p, q = H.ptr(buf), H.ptr(n)
    assert lib.dx_attn_stat_pool_fwd(p, p, q, p, p, 1, max_t + 1, 4, H.stream()) == -5 and b'at most' in lib.dx_last_error()
    assert lib.dx_attn_stat_pool_fwd(p, p, q, p, p, 1, 4, max_c + 1, H.stream()) == -5
    assert lib.dx_attn_stat_pool_bwd(p, p, q, p, p, p, p, p, p, 1, max_t + 1, 4, H.stream()) == -5
    assert lib.dx_attn_stat_pool_bwd(p, p, q, p, p, p, p, p, p, 1, 4, max_c + 1, H.stream()) == -5
    assert lib.dx_attn_stat_pool_fwd(p, None, q, p, p, 1, 4, 4, H.stream()) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_attn_stat_pool_bwd(p, p, q, p, p, p, None, p, p, 1, 4, 4, H.stream()) == -1
    with pytest.raises(ValueError, match='at most'):
        attn_stat_pool(torch.zeros((1, 2, max_c + 1), device=DEV), torch.zeros((1, 2), device=DEV), n[:1])
    torch.cuda.synchronize()


# ---- dx_trial_counts ---------------------------------------------------------------------------------------------------------------------

def _trials(E, spk):
    ''' `dx_trial_counts` with the output poisoned: the entry point clears it '''
    from daft_exprt import _hip as H
    Ed, sd = _dev(np.asarray(E, dtype=np.float32)), _dev(np.asarray(spk, dtype=np.int32))
    counts = torch.full((2, O.BINS), -77, dtype=torch.int64, device=DEV)
    H.check(H.lib().dx_trial_counts(H.ptr(Ed), H.ptr(sd), H.ptr(counts), Ed.shape[0], Ed.shape[1], H.stream()))
    return counts.cpu().numpy()


@pytest.mark.parametrize('D', (64, 200, 20))
def test_trial_counts_are_exact(D):
    ''' rows of 64 entries of +-1/8 (D = 64, 200) or 16 of +-1/4 (D = 20): every partial sum of a dot product is exact in fp32, so
        the counts must EQUAL the float64 oracle's.  N = 1 (no pair), 2, the tile edge 127 / 128 / 129, 300 (six tiles, three of
        them on the diagonal); duplicated rows (s = 1 clamps into the top bin) and negated rows (s = -1: bin 0); 1, 2 and 7
        speakers; everything twice '''
    for N in (1, 2, 127, 128, 129, 300):
        for S in (1, 2, 7):
            E, spk = O.exact_rows(N, D, S)
            want = O.trial_counts(E, spk)
            got, again = _trials(E, spk), _trials(E, spk)
            assert got.tobytes() == again.tobytes()
            assert np.array_equal(got, want), (N, D, S, int(np.abs(got - want).sum()))
            assert got.sum() == N * (N - 1) // 2
            if S == 1:
                assert not got[1].any()
            if N >= 127:
                assert got[:, O.BINS - 1].sum() > 0 and got[:, 0].sum() > 0


def test_trial_counts_over_many_tiles():
    ''' N = 2 049 rows: 17 x 17 tiles, 153 in the upper triangle '''
    E, spk = O.exact_rows(2049, 200, 7)
    want = O.trial_counts(E, spk)
    got, again = _trials(E, spk), _trials(E, spk)
    assert got.tobytes() == again.tobytes() and np.array_equal(got, want)
    assert got.sum() == 2049 * 2048 // 2 and got[0].sum() > 0 and got[1].sum() > 0


@pytest.mark.parametrize('D', (20, 192))
def test_trial_counts_of_random_unit_rows(D):
    ''' a fp32 dot product of unit vectors is within D eps32 of the true value and (s + 1) 2048 adds at most 4 eps32 in units of s:
        with delta = (D + 4) eps32, at every bin edge and in each class the cumulative count differs from the oracle's by at most
        the oracle pairs whose float64 score lies within delta of that edge; the totals are exact '''
    rng = np.random.RandomState(D)
    N = 300
    E = rng.standard_normal((N, D))
    E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32)
    spk = rng.randint(0, 5, size=N).astype(np.int32)
    got = _trials(E, spk)
    scores, same = O.trial_scores(E, spk)
    delta = (D + 4) * EPS
    edges = np.arange(O.BINS + 1) / 2048.0 - 1.0
    worst = 0
    for row, s in ((0, np.sort(scores[same])), (1, np.sort(scores[~same]))):
        assert got[row].sum() == len(s)
        below = np.concatenate([[0], np.cumsum(got[row])])                   # the GPU's pairs in the bins below edge k
        want = np.searchsorted(s, edges, side='left')
        near = np.searchsorted(s, edges + delta, side='right') - np.searchsorted(s, edges - delta, side='left')
        assert (np.abs(below - want) <= near).all(), (row, int(np.abs(below - want).max()))
        worst = max(worst, int(np.abs(below - want).max()))
    print(f'D={D}: {int(got.sum())} trials, the largest cumulative difference at an edge: {worst}')
    assert got.sum() == N * (N - 1) // 2


def test_trial_argument_errors_are_codes():
    from daft_exprt import _hip as H
    from daft_exprt.speaker import limits, trial_counts
    lib = H.lib()
    _, _, max_d, max_n = limits()
    E, spk = torch.zeros((4, 8), device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    counts = torch.zeros((2, O.BINS), dtype=torch.int64, device=DEV)
    assert lib.dx_trial_counts(H.ptr(E), H.ptr(spk), H.ptr(counts), max_n + 1, 8, H.stream()) == -5 and b'at most' in lib.dx_last_error()
    assert lib.dx_trial_counts(H.ptr(E), H.ptr(spk), H.ptr(counts), 4, max_d + 1, H.stream()) == -5
    assert lib.dx_trial_counts(None, H.ptr(spk), H.ptr(counts), 4, 8, H.stream()) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_trial_counts(H.ptr(E), H.ptr(spk), H.ptr(counts), 0, 8, H.stream()) == -2
    with pytest.raises(ValueError, match='at most'):
        trial_counts(torch.zeros((2, max_d + 1), device=DEV), spk[:2])
    E[:, 0] = 1.0
    assert trial_counts(E, spk)[0, O.BINS - 1].item() == 6                   # the wrapper: six pairs of equal rows, one speaker
    torch.cuda.synchronize()


# ---- learnability ------------------------------------------------------------------------------------------------------------------------

def _rates(enc, train, held):
    ''' centroids from the training utterances, then `held_out_report` of the held-out ones '''
    from daft_exprt.speaker import held_out_report, speaker_centroids
    (tmel, tn, tspk), (hmel, hn, hspk) = train, held
    with torch.no_grad():
        enc.set_speakers(list(range(O.TOY['speakers'])), speaker_centroids(enc.embed(tmel, tn), tspk, O.TOY['speakers']))
        emb = enc.embed(hmel, hn)
    report = held_out_report(enc, emb, hspk)
    enc.threshold, enc.eer = report['threshold'], report['eer']
    return report, emb


@functools.lru_cache(maxsize=None)
def _trained():
    ''' (the toy encoder after training, its held-out report before and after, the held-out embeddings), trained once '''
    from daft_exprt.speaker import SpeakerEncoder, am_softmax_loss
    cfg = O.TOY
    train, held = O.toy_corpus()
    train, held = (tuple(t.to(DEV) for t in O.toy_collate(u, torch.float32)) for u in (train, held))
    tmel, tn, tspk = train
    seed = 0
    torch.manual_seed(seed)
    enc = SpeakerEncoder(cfg['n_mel'], hidden=cfg['hidden'], layers=cfg['layers'], stride=cfg['stride'], dim=cfg['dim']).to(DEV)
    weights = torch.nn.Parameter(torch.randn((cfg['speakers'], cfg['dim']), device=DEV))
    enc.eval()
    before, _ = _rates(enc, train, held)
    enc.train()
    opt = torch.optim.Adam(list(enc.parameters()) + [weights], lr=cfg['lr'])
    for idx in O.toy_batches(seed, tmel.shape[0]):
        idx = torch.tensor(idx, device=DEV)
        loss = am_softmax_loss(enc(tmel[idx], tn[idx]), weights, tspk[idx], cfg['scale'], cfg['margin'])
        opt.zero_grad()
        loss.backward()
        opt.step()
    enc.eval()
    after, emb = _rates(enc, train, held)
    return enc, before, after, emb, held, float(loss.detach())


def test_the_encoder_learns_the_toy_speakers():
    ''' 6 speakers x 40 fabricated utterances of 4 to 12 phones (the recogniser's templates, 2 to 7 frames each, 0.3 x Gaussian
        noise) plus a fixed per-channel offset of deviation 0.25 per speaker; 180 train SpeakerEncoder(hidden 64, 2 convolutions,
        stride 2, dim 32) for 300 Adam steps at 3e-3 with 32 utterances each, the other 60 are held out.  The held-out
        identification error and equal error rate must not exceed the ceilings 0.0667 and 0.0740 = the maximum plus the spread of
        `speaker_oracle.toy_restatement` -- plain torch, float64, CPU, the same architecture, loss, data and schedule -- which gave
        identification errors 0.0333, 0.0167, 0, 0, 0, 0 and equal error rates 0.0372, 0.0157, 0.0003, 0.0147, 0.0147, 0.0007 for
        the seeds 0 .. 5 (untrained: 0.35 to 0.47 and 0.41 to 0.46). '''
    enc, before, after, _, _, loss = _trained()
    print(f'held-out identification error: untrained {before["identification_error"]:.4f}, trained {after["identification_error"]:.4f} '
          f'(ceiling {O.CEILING_ID:.4f}); equal error rate: untrained {before["eer"]:.4f}, trained {after["eer"]:.4f} (ceiling '
          f'{O.CEILING_EER:.4f}); threshold {after["threshold"]:.4f}, trials {after["trials"]}, loss {loss:.4f}')
    assert after['trials'] == [6 * 45, 60 * 59 // 2 - 6 * 45] and sum(v['count'] for v in after['per_speaker'].values()) == 60
    assert sum(v['errors'] for v in after['per_speaker'].values()) == round(after['identification_error'] * 60)
    assert before['identification_error'] > 0.2 and before['eer'] > 0.2
    assert after['identification_error'] <= O.CEILING_ID
    assert after['eer'] <= O.CEILING_EER


def test_the_scores_measure_what_they_say():
    ''' the held-out utterances of speaker k scored against speaker (k + 1) mod 6: hardly any is identified as that speaker, the
        margin is negative, and no more are accepted than the equal error rate allows, plus the trials that sit in the threshold's
        own bin (counted by the oracle on the same embeddings) '''
    from daft_exprt.speaker import speaker_scores
    enc, _, after, emb, (hmel, hn, hspk), _ = _trained()
    own = speaker_scores(enc, hmel, hn, hspk)
    wrong = speaker_scores(enc, hmel, hn, ((hspk + 1) % 6).tolist(), reference_embeddings=emb)
    assert tuple(own) == ('cos_target', 'margin', 'identified', 'accepted') and tuple(wrong) == tuple(own) + ('cos_reference',)
    assert all(v.shape == (60,) and v.is_cuda for v in wrong.values())
    assert float((~own['identified']).float().mean()) == pytest.approx(after['identification_error'])
    assert torch.allclose(wrong['cos_reference'], torch.ones(60, device=DEV), atol=1e-5)      # its own embedding as the reference
    counts = O.trial_counts(emb.cpu().numpy(), hspk.cpu().numpy())
    k = round((enc.threshold + 1.0) * 2048)
    in_bin = float(counts[:, k].sum()) / counts.sum() if k < O.BINS else 0.0
    identified, accepted = float(wrong['identified'].float().mean()), float(wrong['accepted'].float().mean())
    print(f'against the next speaker: identified {identified:.4f}, mean margin {float(wrong["margin"].mean()):.4f}, accepted '
          f'{accepted:.4f} (allowed {O.CEILING_EER + in_bin:.4f}); own speaker: mean margin {float(own["margin"].mean()):.4f}, '
          f'accepted {float(own["accepted"].float().mean()):.4f}')
    assert identified <= O.CEILING_ID
    assert float(wrong['margin'].mean()) < 0 < float(own['margin'].mean())
    assert accepted <= O.CEILING_EER + in_bin
    unknown = speaker_scores(enc, hmel[:2], torch.tensor([0, 5], device=DEV), [0, 99])        # no frame; a speaker it never saw
    assert torch.isnan(unknown['cos_target']).all() and not unknown['identified'].any() and not unknown['accepted'].any()


# ---- the command lines, end to end -------------------------------------------------------------------------------------------------------

REPORT_KEYS = ('utterances_train', 'utterances_held_out', 'speakers', 'steps', 'loss', 'identification_error', 'eer', 'threshold',
               'trials', 'per_speaker', 'left_out')


def _script(name, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', f'{name}.py'), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def _cli(name):
    ''' a script as a module: `main(argv)` in this process, which has the GPU open and torch imported already '''
    spec = importlib.util.spec_from_file_location(f'{name}_cli', os.path.join(ROOT, 'scripts', f'{name}.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _checkpoint_and_encoder(golden_dir, tmp_path, steps):
    ''' a tiny acoustic model's checkpoint, the file list of tests/golden (speakers 0, 3, 7) and an encoder trained on it '''
    from tests.test_gpu_dtw import _file_list, _tiny_model
    model, hp = _tiny_model(golden_dir)
    ckpt = str(tmp_path / 'DaftExprt_test')
    torch.save({'iteration': 0, 'state_dict': {f'module.{k}': v for k, v in model.state_dict().items()}, 'config_params': dict(vars(hp))}, ckpt)
    list_file, names, speakers = _file_list(golden_dir, tmp_path)
    spk_path = str(tmp_path / 'speaker.pt')
    report = _cli('train_speaker_encoder').main(['-chk', ckpt, '-tf', list_file, '-vf', list_file, '-o', spk_path, '-st', str(steps), '-bs', '4',
                                                 '-hid', '32', '-ly', '2', '-dim', '16', '--margin', '0.1', '--scale', '20', '--seed', '3'])
    return hp, ckpt, list_file, names, speakers, spk_path, report


def _check_scores(entry, reference=False):
    from daft_exprt.speaker import REFERENCE_KEY, SPEAKER_KEYS
    assert tuple(entry) == SPEAKER_KEYS + ((REFERENCE_KEY,) if reference else ())
    assert -1.0001 <= entry['cos_target'] <= 1.0001 and np.isfinite(entry['margin'])
    assert isinstance(entry['identified'], bool) and isinstance(entry['accepted'], bool) and entry['identified'] == (entry['margin'] > 0)


def test_train_speaker_encoder_then_evaluate_with_it(golden_dir, tmp_path):
    from daft_exprt.evaluate import SPEAKER_LEVELS
    from daft_exprt.speaker import SPEAKER_KEYS, SpeakerEncoder, load_speaker_encoder
    hp, ckpt, list_file, names, speakers, spk_path, returned = _checkpoint_and_encoder(golden_dir, tmp_path, 30)
    report = json.load(open(tmp_path / 'speaker_report.json'))
    assert json.loads(json.dumps(returned)) == report and tuple(report) == REPORT_KEYS
    assert report['utterances_train'] == 5 == report['utterances_held_out'] and report['speakers'] == 3 and report['left_out'] == 0
    assert report['steps'] == 30 and np.isfinite(report['loss']) and 0 <= report['identification_error'] <= 1
    assert report['trials'] == [2, 8] and 0 <= report['eer'] <= 1 and -1 <= report['threshold'] <= 1
    assert {k: v['count'] for k, v in report['per_speaker'].items()} == {'0': 2, '3': 2, '7': 1}
    enc = load_speaker_encoder(spk_path)
    assert isinstance(enc, SpeakerEncoder) and all(p.is_cuda and torch.isfinite(p).all() for p in enc.parameters())
    assert enc.args == dict(n_mel=hp.n_mel_channels, hidden=32, layers=2, stride=2, dim=16) and enc.speaker_ids == [0, 3, 7]
    assert enc.centroids.shape == (3, 16) and enc.centroids.is_cuda and (enc.threshold, enc.eer) == (report['threshold'], report['eer'])
    plain, scored = str(tmp_path / 'plain'), str(tmp_path / 'scored')
    evaluate = _cli('evaluate')
    evaluate.main(['-chk', ckpt, '-vf', list_file, '-out', plain])
    evaluate.main(['-chk', ckpt, '-vf', list_file, '-out', scored, '-spk', spk_path])
    a, b = (json.load(open(os.path.join(d, 'copy_synthesis.json'))) for d in (plain, scored))
    assert list(a) == ['audio', 'files', 'summary'] and all(list(e) == ['speaker_id', 'mel', 'audio'] for e in a['files'].values())
    assert list(a['summary']) == ['files', 'mel', 'audio', 'speakers'] and all(list(s) == ['files', 'mel', 'audio'] for s in a['summary']['speakers'].values())
    for name in names:                                                       # -spk adds `speaker` and changes nothing else
        entry = dict(b['files'][name])
        speaker = entry.pop('speaker')
        assert entry == a['files'][name] and tuple(speaker) == SPEAKER_LEVELS == ('recording', 'mel', 'audio')
        for level in SPEAKER_LEVELS:
            _check_scores(speaker[level])
    for table in [b['summary']] + list(b['summary']['speakers'].values()):
        assert tuple(table['speaker']) == SPEAKER_LEVELS
        for level in SPEAKER_LEVELS:
            s = table['speaker'][level]
            assert set(s) == set(SPEAKER_KEYS) and s['cos_target']['count'] == table['files'] and 0 <= s['identified'] <= 1 and 0 <= s['accepted'] <= 1
    stripped = json.loads(json.dumps(b['summary']))
    for table in [stripped] + list(stripped['speakers'].values()):
        del table['speaker']
    assert stripped == a['summary']
    want = sum(b['files'][n]['speaker']['audio']['identified'] for n in names) / len(names)
    assert b['summary']['speaker']['audio']['identified'] == pytest.approx(want)


def test_synthesize_with_a_speaker_encoder_writes_speaker_identity(golden_dir, tmp_path):
    ''' `scripts/synthesize.py -spk S` (a script that takes its arguments from the command line only: two child processes) '''
    from tests.test_gpu_prosody_eval import _style_bank
    hp, ckpt, _, _, _, spk_path, _ = _checkpoint_and_encoder(golden_dir, tmp_path, 3)
    bank = str(tmp_path / 'bank')
    _style_bank(bank, hp)
    text = tmp_path / 'sentences_to_generate.txt'
    text.write_text('s.txt_line0|{HH AH0 L OW1} {W ER1 L D} , {T EH1 S T} ? ~\ns.txt_line1|{T EH1 S T} . ~\n', encoding='utf-8')
    outs = []
    for out_dir, extra in ((str(tmp_path / 'syn_plain'), ()), (str(tmp_path / 'syn_scored'), ('-spk', spk_path))):
        _script('synthesize', '-out', out_dir, '-chk', ckpt, '-tf', str(text), '-sb', bank, '-bs', '2', *extra)
        outs.append(out_dir)
    assert not os.path.exists(os.path.join(outs[0], 'speaker_identity.json'))
    assert sorted(f for f in os.listdir(outs[0]) if f.endswith('.json')) == ['prosody_transfer.json']
    a, b = (json.load(open(os.path.join(d, 'prosody_transfer.json'))) for d in outs)
    assert a == b                                                            # the same seed, the same audio, the same report
    report = json.load(open(os.path.join(outs[1], 'speaker_identity.json')))
    assert list(report) == ['audio', 'files', 'summary'] and report['audio'] == 'griffin-lim' and sorted(report['files']) == sorted(b['files'])
    for name, entry in report['files'].items():
        entry = dict(entry)
        assert entry.pop('wav') == b['files'][name]['wav'] and os.path.isfile(os.path.join(outs[1], b['files'][name]['wav']))
        requested = entry.pop('speaker_id')
        assert f'_spk_{requested}_ref_' in name and isinstance(entry.pop('reference'), str)
        assert entry.pop('reference_identified_as') in (0, 3, 7)
        assert -1.0001 <= entry['cos_reference'] <= 1.0001
        if requested in (0, 3, 7):
            _check_scores(entry, reference=True)
        else:       # the script draws from the acoustic model's 11 speakers; the encoder was trained on three: no centroid, no score
            assert tuple(entry) == ('cos_target', 'margin', 'identified', 'accepted', 'cos_reference')
            assert entry['cos_target'] is None and entry['margin'] is None and not entry['identified'] and not entry['accepted']
    s = report['summary']
    assert list(s) == ['files', 'identified', 'accepted', 'other_reference', 'target_minus_reference', 'leaked']
    assert s['files'] == 2 and s['identified'] == sum(e['identified'] for e in report['files'].values()) / 2
    other = [e for e in report['files'].values() if e['reference_identified_as'] != e['speaker_id'] and e['cos_target'] is not None]
    assert s['other_reference'] == len(other)
    if other:
        assert s['target_minus_reference'] == pytest.approx(sum(e['cos_target'] - e['cos_reference'] for e in other) / len(other))
        assert s['leaked'] == sum(e['cos_target'] < e['cos_reference'] for e in other) / len(other)
    else:
        assert s['target_minus_reference'] is None and s['leaked'] is None
