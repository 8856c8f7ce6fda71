"""tests/aligner_oracle.py pinned without a GPU: the float64 restatement of K28 against brute force over every monotone path,
against torch float64 autograd of a restated recursion, and against hand-worked lattices for the tie rule; what of
daft_exprt/aligner.py and scripts/train_aligner.py can be told on the host."""
import inspect
import itertools
import os

import numpy as np
import pytest
import torch

from tests import aligner_oracle as O

FLOOR = -1e30        # in place of -inf in the torch restatement: torch.logaddexp's backward gives NaN at (-inf, -inf)


def _lattice(T, L, seed):
    return -np.random.RandomState(seed).uniform(0.1, 4.0, size=(1, T, L))


def _lse(values):
    values = np.asarray(values, dtype=np.float64)
    return values.max() + np.log(np.exp(values - values.max()).sum())


@pytest.mark.parametrize('T,L', [(T, L) for T in range(1, 8) for L in range(1, 5) if L <= T])
def test_every_monotone_path_enumerated(T, L):
    logp = _lattice(T, L, 100 * T + L)
    paths = O.monotone_paths(T, L)
    assert len(paths) > 0 and all(p[0] == 0 and p[-1] == L - 1 and all(0 <= b - a <= 1 for a, b in zip(p, p[1:])) for p in paths)
    scores = np.array([sum(logp[0, t, l] for t, l in enumerate(p)) for p in paths])
    n = [np.array([T]), np.array([L])]
    alpha, loss, status = O.forward_sum(logp, *n)
    assert status[0] == 0 and abs(loss[0] + _lse(scores)) < 1e-12
    post = np.exp(scores - _lse(scores))
    occupancy = np.zeros((T, L))
    for p, w in zip(paths, post):
        for t, l in enumerate(p):
            occupancy[t, l] += w
    gamma = O.forward_sum_bwd(logp, alpha, np.ones(1), *n, return_gamma=True)[0]
    assert np.abs(gamma - occupancy).max() < 1e-12
    assert (gamma[occupancy == 0] == 0).all()                          # cells no path visits: exactly 0
    assert np.abs(gamma.sum(axis=1) - 1).max() < 1e-12
    dlogp = O.forward_sum_bwd(logp, alpha, np.array([0.7]), *n)[0]
    assert np.abs(dlogp + 0.7 * occupancy).max() < 1e-12
    path, path_len, score, st = O.mas(logp, *n)
    assert st[0] == 0 and path_len[0] == T and abs(score[0] - scores.max()) < 1e-12
    got = path[0, :T, 1].tolist()
    assert path[0, :T, 0].tolist() == list(range(T)) and (path[0, T:] == -1).all()
    assert got in paths and abs(scores[paths.index(got)] - scores.max()) < 1e-12


def test_statuses_and_dead_rows():
    logp = np.full((4, 5, 3), np.nan)
    logp[0, :2, :3] = -1.0
    logp[3, :5, :3] = -1.0
    n_frm, n_sym = np.array([2, 0, 4, 5]), np.array([3, 2, 0, 3])
    alpha, loss, status = O.forward_sum(logp, n_frm, n_sym)
    assert status.tolist() == [1, 2, 2, 0] and np.isnan(loss[:3]).all() and not alpha[:3].any() and np.isfinite(loss[3])
    assert not O.forward_sum_bwd(logp, alpha, np.ones(4), n_frm, n_sym)[:3].any()
    path, path_len, score, st = O.mas(logp, n_frm, n_sym)
    assert st.tolist() == [1, 2, 2, 0] and path_len.tolist() == [0, 0, 0, 5] and (path[:3] == -1).all() and np.isnan(score[:3]).all()
    assert np.isneginf(O.logaddexp(-np.inf, -np.inf)) and O.logaddexp(-np.inf, 2.0) == 2.0
    assert np.isneginf(alpha[3, 0, 1:]).all() and np.isneginf(alpha[3, 1, 2])


# ---- the tie rule, worked by hand ------------------------------------------------------------------------------------------------------
# (t - 1, l) is the predecessor unless (t - 1, l - 1) is STRICTLY greater: among equal paths the one that enters every symbol as early
# as the forced diagonal allows is returned.
TIE_CASES = (
    # all zeros, 3 x 2: V(1) = [0, 0]; at (2, 1) left 0 is not > 0: stay; at (1, 1) t = l: forced step
    ('zeros-3x2', np.zeros((3, 2)), [0, 1, 1], 0.0),
    ('zeros-4x2', np.zeros((4, 2)), [0, 1, 1, 1], 0.0),
    # logp(1, 1) = -1: V(1) = [0, -1]; at (2, 1) left 0 > -1: step; at (3, 1) left 0 is not > V(2, 1) = 0: stay
    ('late-entry', np.array([[0., 0.], [0., -1.], [0., 0.], [0., 0.]]), [0, 0, 1, 1], 0.0),
    # the forced diagonal: 3 x 3 has one path whatever the values
    ('diagonal', np.array([[0., 9., 9.], [9., -5., 9.], [9., 9., -5.]]), [0, 1, 2], -10.0),
    # zeros 5 x 3: (4, 2) stays, (3, 2) stays, (2, 2) forced, (1, 1) forced
    ('zeros-5x3', np.zeros((5, 3)), [0, 1, 2, 2, 2], 0.0),
    # one symbol: every frame is its
    ('one-symbol', -np.ones((4, 1)), [0, 0, 0, 0], -4.0),
)


@pytest.mark.parametrize('name,logp,labels,score', TIE_CASES, ids=[c[0] for c in TIE_CASES])
def test_tie_rule_on_hand_built_lattices(name, logp, labels, score):
    T, L = logp.shape
    path, path_len, got, status = O.mas(logp[None], np.array([T]), np.array([L]))
    assert status[0] == 0 and path_len[0] == T and path[0, :T, 1].tolist() == labels and got[0] == score
    assert O.durations_of_path(path, path_len, [L], L)[0].tolist() == np.bincount(labels, minlength=L).tolist()
    for dtype in (np.float32,):
        assert O.mas(logp[None], np.array([T]), np.array([L]), dtype)[0][0, :T, 1].tolist() == labels


# ---- gradients against torch float64 autograd of a restated recursion -------------------------------------------------------------------

def _torch_loss(q, k, n_frm, n_sym, temperature, prior_sigma, w):
    total, logps = 0., []
    for b in range(q.shape[0]):
        nf, ns = int(n_frm[b]), int(n_sym[b])
        d = ((q[b, :nf, None, :] - k[b, None, :ns, :]) ** 2).sum(-1)
        s = -temperature * d + torch.from_numpy(O.prior(nf, ns, prior_sigma))
        logp = torch.log_softmax(s, dim=1)
        logp.retain_grad()
        logps.append(logp)
        a = torch.full((ns,), FLOOR, dtype=torch.float64)
        a = torch.cat([logp[0, :1], a[1:]])
        for t in range(1, nf):
            a = logp[t] + torch.logaddexp(a, torch.cat([torch.full((1,), FLOOR, dtype=torch.float64), a[:-1]]))
        total = total - w[b] * a[ns - 1]
    return total, logps


@pytest.mark.parametrize('prior_sigma', [0.0, 0.3])
def test_gradients_equal_torch_float64_autograd(prior_sigma):
    rng = np.random.RandomState(5)
    shapes, A, tau = [(1, 1), (2, 1), (5, 5), (9, 2), (12, 7)], 6, 0.3
    B, T, L = len(shapes), max(s[0] for s in shapes), max(s[1] for s in shapes)
    n_frm, n_sym = np.array([s[0] for s in shapes]), np.array([s[1] for s in shapes])
    q, k, w = rng.standard_normal((B, T, A)), rng.standard_normal((B, L, A)), rng.uniform(0.5, 2.0, size=B)
    tq, tk = torch.from_numpy(q).requires_grad_(), torch.from_numpy(k).requires_grad_()
    total, logps = _torch_loss(tq, tk, n_frm, n_sym, tau, prior_sigma, w)
    total.backward()

    logp = O.logprob_fwd(q, k, n_frm, n_sym, tau, prior_sigma)
    alpha, loss, status = O.forward_sum(logp, n_frm, n_sym)
    assert not status.any() and abs(float(total.detach()) - float((w * loss).sum())) < 1e-10
    dlogp = O.forward_sum_bwd(logp, alpha, w, n_frm, n_sym)
    dq, dk = O.logprob_bwd(q, k, logp, dlogp, n_frm, n_sym, tau)
    for b, (nf, ns) in enumerate(shapes):
        assert np.abs(logp[b, :nf, :ns] - logps[b].detach().numpy()).max() < 1e-12
        assert np.abs(dlogp[b, :nf, :ns] - logps[b].grad.numpy()).max() < 1e-10
        assert not dlogp[b, nf:].any() and not dlogp[b, :, ns:].any() and not logp[b, nf:].any() and not logp[b, :, ns:].any()
    # rows and keys past the lengths got no gradient from torch either
    assert np.abs(dq - tq.grad.numpy()).max() < 1e-10 and np.abs(dk - tk.grad.numpy()).max() < 1e-10
    assert np.abs(np.exp(logp[0, :1, :1]).sum() - 1) < 1e-12 and np.abs(np.exp(logp[4, :12, :7]).sum(axis=1) - 1).max() < 1e-12


def test_float32_restatement_is_close_and_in_float32():
    rng = np.random.RandomState(6)
    q, k = rng.standard_normal((2, 40, 8)), rng.standard_normal((2, 9, 8))
    n_frm, n_sym = np.array([40, 17]), np.array([9, 4])
    hi, lo = O.logprob_fwd(q, k, n_frm, n_sym, 0.2, 0.5), O.logprob_fwd(q, k, n_frm, n_sym, 0.2, 0.5, np.float32)
    assert lo.dtype == np.float32 and 0 < np.abs(hi - lo).max() < 1e-4
    a_hi, l_hi, _ = O.forward_sum(hi, n_frm, n_sym)
    a_lo, l_lo, _ = O.forward_sum(hi, n_frm, n_sym, np.float32)
    assert a_lo.dtype == np.float32 and np.abs(l_hi - l_lo).max() < 1e-3
    g = O.forward_sum_bwd(hi, a_hi, np.ones(2), n_frm, n_sym, np.float32)
    assert g.dtype == np.float32 and np.abs(g - O.forward_sum_bwd(hi, a_hi, np.ones(2), n_frm, n_sym)).max() < 1e-3


# ---- the toy corpus of the learnability test ---------------------------------------------------------------------------------------------

def test_toy_corpus_is_as_the_issue_describes_it():
    utts = O.toy_corpus()
    assert len(utts) == 64
    for sym, dur, mel in utts:
        assert 4 <= len(sym) <= 12 and int(sym.min()) >= 1 and int(sym.max()) <= 15 and (sym[1:] != sym[:-1]).all()
        assert int(dur.min()) >= 2 and int(dur.max()) <= 7 and mel.shape == (int(dur.sum()), 80)
    assert len(O.toy_batches(0)) == 150 and all(len(b) == 32 for b in O.toy_batches(0))


# ---- daft_exprt/aligner.py on the host ------------------------------------------------------------------------------------------------

def test_aligner_module_on_the_host(tmp_path):
    from daft_exprt import align
    from daft_exprt.aligner import Aligner, load_aligner, save_aligner
    torch.manual_seed(0)
    model = Aligner(n_symbols=11, n_mel=8, hidden=16, att_dim=4, temperature=0.1, prior_sigma=0.3)
    symbols = torch.randint(1, 11, (2, 6))
    mel = torch.randn(2, 8, 13)
    n_sym, n_frm = torch.tensor([6, 3]), torch.tensor([13, 7])
    q, k = model.encode(symbols, n_sym, mel, n_frm)
    assert q.shape == (2, 13, 4) and k.shape == (2, 6, 4) and q.dtype == torch.float32 and q.is_contiguous() and k.is_contiguous()
    # masked at the sequence ends: what lies past an utterance's end does not reach its live rows
    q1, k1 = model.encode(symbols[1:, :3], n_sym[1:], mel[1:, :, :7], n_frm[1:])
    assert torch.equal(q1[0], q[1, :7]) and torch.equal(k1[0], k[1, :3])
    # the convolutions stated as matrix products are torch's Conv1d
    x = torch.randn(2, 13, 16)
    want = model.query_2(x.transpose(1, 2)).transpose(1, 2)
    from daft_exprt.aligner import _conv
    assert (want - _conv(x, model.query_2)).abs().max() < 1e-5
    # checkpoints: the weights and the constructor arguments
    save_aligner(model, str(tmp_path / 'aligner.pt'))
    again = load_aligner(str(tmp_path / 'aligner.pt'), device='cpu')
    assert again.args == model.args and again.temperature == 0.1 and again.prior_sigma == 0.3
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), again.state_dict().values()))
    # the same call as align.align_batch after the model, and no CPU fallback
    theirs = list(inspect.signature(align.align_batch).parameters)[1:]
    assert list(inspect.signature(model.align_batch).parameters) == theirs
    with pytest.raises(RuntimeError):
        model.align_batch(symbols, n_sym, torch.zeros(2, 4000), [4000, 4000], torch.zeros(2, dtype=torch.int64), None)
    with pytest.raises(RuntimeError):
        model(symbols, n_sym, mel, n_frm)


def test_header_declares_the_limits_the_issue_asks_for():
    from daft_exprt import _hip as H
    lib = H.lib()
    assert lib.dx_aln_max_symbols() >= 512 and lib.dx_aln_max_dim() >= 128
    p = 8
    assert lib.dx_aln_forward_sum(None, p, p, p, p, p, 1, 2, 2, None) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_aln_forward_sum(p, p, p, p, p, p, 1, 0, 2, None) == -2
    assert lib.dx_aln_forward_sum(p, p, p, p, p, p, 1, lib.dx_dtw_max_len() + 1, 2, None) == -5
    assert lib.dx_aln_mas(p, p, p, p, p, p, p, p, 64, 1, 2, lib.dx_aln_max_symbols() + 1, None) == -5
    assert lib.dx_aln_logprob_fwd(p, p, p, p, 1.0, 0.0, p, 1, 2, 2, lib.dx_aln_max_dim() + 1, None) == -5
    assert lib.dx_aln_logprob_fwd(p, p, p, p, 0.0, 0.0, p, 1, 2, 2, 2, None) == -1 and b'temperature' in lib.dx_last_error()
    assert lib.dx_aln_mas(p, p, p, p, p, p, p, p, 8, 1, 2, 2, None) == -2 and b'ws_stride' in lib.dx_last_error()


def test_train_aligner_cli_argument_checks(tmp_path):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('train_aligner_cli', os.path.join(root, 'scripts', 'train_aligner.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    text = tmp_path / 'sentences.txt'
    text.write_text('u0|{HH AH0} ~\n', encoding='utf-8')
    base = ['-dd', str(tmp_path), '-o', str(tmp_path / 'aligner.pt')]
    args = cli.parse_args(base + ['-spks', 'A', 'B', '-tf', str(text)])
    assert (args.speakers, args.text_file, args.steps, args.batch_size, args.learning_rate, args.min_frames, args.trim_db, args.overwrite) == \
        (['A', 'B'], [str(text)], 2000, 32, 1e-3, 3, -40.0, False)
    cli.check_args(args)
    args = cli.parse_args(base + ['-spks', 'A', '-tf', str(text), '-st', '10', '-bs', '4', '-lr', '0.01', '-mf', '2', '-trim', '-30', '--overwrite'])
    assert (args.steps, args.batch_size, args.learning_rate, args.min_frames, args.trim_db, args.overwrite) == (10, 4, 0.01, 2, -30.0, True)
    cli.check_args(args)
    for bad, word in ((['-tf', str(text), str(text), str(text)], 'one per speaker'), (['-tf', str(tmp_path / 'none.txt')], 'no such phonemised'),
                      (['-tf', str(text), '-mf', '0'], 'at least 1'), (['-tf', str(text), '-trim', '3'], 'at most 0'),
                      (['-tf', str(text), '-st', '0'], 'at least 1'), (['-tf', str(text), '-lr', '0'], 'positive'),
                      (['-tf', str(text), '-o', str(tmp_path / 'none' / 'a.pt')], 'no such directory for -o')):
        with pytest.raises(SystemExit) as e:
            cli.check_args(cli.parse_args(base + ['-spks', 'A', 'B'] + bad))
        assert word in str(e.value), (bad, str(e.value))
    with pytest.raises(SystemExit) as e:
        cli.check_args(cli.parse_args(['-dd', str(tmp_path / 'none'), '-o', str(tmp_path / 'a.pt'), '-spks', 'A', '-tf', str(text)]))
    assert 'no such data set directory' in str(e.value)
