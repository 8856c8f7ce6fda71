"""K31 (csrc/recognizer.hip) and daft_exprt/recognizer.py on the GPU against tests/ctc_oracle.py and tests/recognizer_oracle.py.

The float outputs of `dx_uctc_loss` are compared with the float64 oracle of K30's mathematics on the same (fp32-representable)
inputs under the project's measured bound, `_bound` of tests/test_gpu_g2p.py, imported: 4 x the deviation of the float32
restatement of the same recurrence from float64 on the same inputs, with a floor of 8 fp32 ulps of the scale.  The greedy decode
and the edit distance are integer results and must equal their oracles exactly.  Every launch gets its dead inputs as NaN /
garbage and its outputs and workspace pre-filled with NaN / garbage, and every row is run in the ragged batch, in a batch with
larger padded extents, and alone: the three must agree bit for bit."""
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

from tests import ctc_oracle as C
from tests import recognizer_oracle as O
from tests.test_gpu_g2p import EPS, _bound, _close, _dev

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- dx_uctc_loss ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(V, which):
    ''' a ragged batch of `recognizer_oracle.uctc_case`, the float64 oracle and the float32 restatement, computed once '''
    c = O.uctc_case(V, which)
    for tag, dt in (('hi', np.float64), ('lo', np.float32)):
        c['loss_' + tag], status, c['grad_' + tag] = C.ctc_loss(c['logits'], c['n_steps'], c['labels'], c['n_labels'], c['w'], dt)
        assert status.tolist() == c['status'].tolist()
    return c


def _run(c, rows=None, pad=(0, 0, 0), entry='dx_uctc_loss'):
    ''' the loss kernel on the rows `rows` of a case (all by default) with the tight extents plus `pad` = (T, U, B): logits at or past
        n_steps NaN, labels at or past n_labels garbage, the padded batch rows without steps; outputs and workspace poisoned '''
    from daft_exprt import _hip as H
    rows = list(range(c['B'])) if rows is None else rows
    n_steps, n_labels = c['n_steps'][rows], c['n_labels'][rows]
    B, V = len(rows) + pad[2], c['V']
    T, U = max(1, int(n_steps.max())) + pad[0], int(n_labels.max()) + pad[1]
    logits = np.full((B, T, V), np.nan, dtype=np.float32)
    labels = np.full((B, max(U, 1)), -7, dtype=np.int64)
    nT, nL, w = np.zeros((B,), dtype=np.int64), np.zeros((B,), dtype=np.int64), np.ones((B,), dtype=np.float32)
    for i, b in enumerate(rows):
        logits[i, :n_steps[i]] = c['logits'][b, :n_steps[i]]
        labels[i, :n_labels[i]] = c['labels'][b, :n_labels[i]]
        labels[i, n_labels[i]:] = 10 ** 6
        nT[i], nL[i], w[i] = n_steps[i], n_labels[i], c['w'][b]
    labels = np.ascontiguousarray(labels[:, :U]) if U else labels[:, :0]
    x, lab, nT, nL, w = _dev(logits), (_dev(labels) if U else None), _dev(nT), _dev(nL), _dev(w)
    o = dict(loss=torch.full((B,), float('nan'), device=DEV), status=torch.full((B,), -77, dtype=torch.int32, device=DEV),
             grad=torch.full((B, T, V), float('nan'), device=DEV))
    ws = torch.full((2 if entry == 'dx_uctc_loss' else 1, B, T, 2 * U + 1), float('nan'), device=DEV)
    H.check(getattr(H.lib(), entry)(H.ptr(x), H.ptr(nT), H.ptr(lab), H.ptr(nL), H.ptr(w), H.ptr(o['loss']), H.ptr(o['status']),
                                    H.ptr(o['grad']), H.ptr(ws), B, T, U, V, H.stream()))
    return {name: t.cpu().numpy() for name, t in o.items()}


def _row(out, i, nT):
    ''' the bytes of row i of an output of `_run`, after checking that its steps at or past n_steps are +0 '''
    g = out['grad'][i]
    assert not g[nT:].any() and not np.signbit(g[nT:]).any()
    return out['loss'][i].tobytes() + out['status'][i].tobytes() + g[:nT].tobytes()


@pytest.mark.parametrize('which', ('short', 'long'))
@pytest.mark.parametrize('V', O.CLASSES)
def test_loss_and_gradient_against_float64_alone_in_a_batch_and_padded(V, which):
    ''' The rows of `recognizer_oracle.SHORT` (lane edges of 1 and 2 states per lane, the steps around K30's limit, a single-path
        row, the statuses 1, 2, 3) and `LONG` (lane edges of 4 and 8 states per lane, 2048 steps x 255 labels).
        Measured on the CPU (float32 restatement against float64, the same inputs): the largest deviation over the rows of the
        case, at the row where it occurs, and the bound that row gets (4 x the deviation; the floor decides the short rows):
          V = 2   short: loss 2.2e-05 -> bound 8.8e-05 (255 x 32),    gradient 3.0e-05 -> 1.2e-04 (61 x 31, the single path)
          V = 2   long:  loss 7.1e-05 -> bound 2.9e-04 (253 x 127),   gradient 2.6e-04 -> 1.0e-03 (2048 x 255)
          V = 65  short: loss 2.9e-04 -> bound 1.2e-03 (256 x 63),    gradient 4.8e-04 -> 1.9e-03 (256 x 63)
          V = 65  long:  loss 1.1e-02 -> bound 4.5e-02 (2048 x 255, |loss| 9.4e+03),  gradient 9.9e-03 -> 4.0e-02 (2048 x 255)
          V = 128 short: loss 1.1e-04 -> bound 1.2e-03 (257 x 64, the floor at |loss| 1.2e+03),  gradient 1.6e-03 -> 6.3e-03 (257 x 64)
          V = 128 long:  loss 2.5e-02 -> bound 1.0e-01 (2048 x 255, |loss| 1.1e+04),  gradient 5.9e-02 -> 2.3e-01 (2048 x 255)
        At 2048 steps of 2 x normal logits the alphas reach 1e+04, where a float32 holds 1e-03: the posteriors exp(alpha + beta -
        log p) of ANY fp32 recursion carry percents there, the restatement's as the kernel's.  Measured on an MI355X, the kernel's
        own worst deviations from float64 at those rows: loss 6.0e-05, 1.1e-02, 2.4e-02 and gradient 2.2e-04, 9.9e-03, 5.7e-02 for
        V = 2, 65, 128 -- 0.16 to 0.25 of their bounds; over all rows the largest ratio of deviation to bound was 0.40 (loss, V = 2,
        600 x 128) and 0.29 (gradient, V = 65, 700 x 191), and on every row that K30 admits K31 gave K30's bits.
        The test prints every row's own figures.  Where K30 admits a row (at most 256 steps and 127 labels) K31 must also be
        within that row's bound of K30's result; it need not equal it bit for bit. '''
    c = _case(V, which)
    shapes = list(zip(c['n_steps'].tolist(), c['n_labels'].tolist()))
    max_t, max_u = 2048, 255
    batch, again = _run(c), _run(c)
    for name in batch:                                                       # two runs: bit-equal
        assert batch[name].tobytes() == again[name].tobytes(), name
    assert batch['status'].tolist() == c['status'].tolist()
    pad = (3, 66, 2) if which == 'short' else (3, 5, 2)                      # every extent larger; short: 4 -> 8 states per lane
    inner = [b for b, (nT, nL) in enumerate(shapes) if nT + pad[0] <= max_t and nL + pad[1] <= max_u]
    wide = _run(c, rows=inner, pad=pad)
    assert wide['status'][len(inner):].tolist() == [2, 2] and np.isnan(wide['loss'][len(inner):]).all()
    assert not wide['grad'][len(inner):].any()
    k30_rows = [b for b, (nT, nL) in enumerate(shapes) if nT <= 256 and nL <= 127]
    k30 = _run(c, rows=k30_rows, entry='dx_ctc_loss') if which == 'short' else None
    for b, (nT, nL) in enumerate(shapes):
        alone = _run(c, rows=[b])
        assert _row(batch, b, nT) == _row(alone, 0, nT), (V, nT, nL)
        if b in inner:
            assert _row(batch, b, nT) == _row(wide, inner.index(b), nT), (V, nT, nL)
        tag = f'V={V} {nT}x{nL} '
        if c['status'][b] != 0:
            assert np.isnan(batch['loss'][b]) and not batch['grad'][b].any()
            continue
        hi, lo, w = c['loss_hi'][b], c['loss_lo'][b], float(c['w'][b])
        largest = float(np.abs(c['logits'][b, :nT]).max())
        loss_bound = _bound(hi, lo, max(abs(hi), largest))
        grad_bound = _bound(c['grad_hi'][b, :nT], c['grad_lo'][b, :nT], largest * w)
        _close(tag + 'loss', batch['loss'][b], hi, loss_bound)
        _close(tag + 'grad', batch['grad'][b, :nT], c['grad_hi'][b, :nT], grad_bound)
        assert not batch['grad'][b, nT:].any()
        if k30 is not None and b in k30_rows:
            i = k30_rows.index(b)
            assert k30['status'][i] == 0
            _close(tag + 'loss against K30', batch['loss'][b], k30['loss'][i], loss_bound)
            _close(tag + 'grad against K30', batch['grad'][b, :nT], k30['grad'][i, :nT], grad_bound)


def test_a_label_out_of_range_is_a_status_not_a_fault():
    from daft_exprt.recognizer import uctc_loss_and_grad
    x = torch.zeros((3, 4, 5), device=DEV)
    labels = torch.tensor([[1, 5], [0, 1], [4, 4]], device=DEV)
    loss, status, grad = uctc_loss_and_grad(x, torch.tensor([4, 4, 4], device=DEV), labels, torch.tensor([2, 1, 2], device=DEV))
    assert status.tolist() == [3, 3, 0] and torch.isnan(loss[:2]).all() and not grad[:2].any() and torch.isfinite(loss[2])
    with pytest.raises(ValueError, match='at most'):
        uctc_loss_and_grad(torch.zeros((1, 2049, 5), device=DEV), torch.tensor([4], device=DEV), labels[:1], torch.tensor([2], device=DEV))


# ---- dx_uctc_greedy ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('V', O.CLASSES)
def test_greedy_decode_is_exact(V):
    from daft_exprt import _hip as H
    x, n_steps = O.greedy_case(V)
    B, T = x.shape[:2]
    want_ids, want_n, score_hi = C.greedy(x, n_steps)
    score_lo = C.greedy(x, n_steps, np.float32)[2]
    ties = sum(int((np.sort(x[b, :n], axis=1)[:, -1] == np.sort(x[b, :n], axis=1)[:, -2]).sum()) for b, n in enumerate(n_steps))
    assert ties > 200
    outs = []
    for shorter, extra in ((0, 0), (0, 0), (1, 1)):                          # twice as it is; then the limit row dropped, T and B padded
        rows = B - shorter
        Tp = int(n_steps[:rows].max()) + 7 * extra
        xp = np.full((rows + extra, Tp, V), np.nan, dtype=np.float32)
        nT = np.zeros((rows + extra,), dtype=np.int64)
        nT[:rows] = n_steps[:rows]
        for b in range(rows):
            xp[b, :n_steps[b]] = x[b, :n_steps[b]]
        o = dict(ids=torch.full(xp.shape[:2], -77, dtype=torch.int32, device=DEV), n_out=torch.full((len(nT),), -77, dtype=torch.int32, device=DEV),
                 score=torch.full((len(nT),), float('nan'), device=DEV))
        xd, nd = _dev(xp), _dev(nT)                                          # (held until the launch has its pointers)
        H.check(H.lib().dx_uctc_greedy(H.ptr(xd), H.ptr(nd), H.ptr(o['ids']), H.ptr(o['n_out']), H.ptr(o['score']), len(nT), Tp, V, H.stream()))
        outs.append(({k: v.cpu().numpy() for k, v in o.items()}, rows, Tp))
    for got, rows, Tp in outs:
        assert got['n_out'][:rows].tolist() == want_n[:rows].tolist()
        assert np.array_equal(got['ids'][:rows, :min(T, Tp)], want_ids[:rows, :Tp]) and not got['ids'][:rows, T:].any()   # zero-filled behind n_out
        assert not got['ids'][rows:].any() and not got['n_out'][rows:].any()
        assert got['score'][:rows].tobytes() == outs[0][0]['score'][:rows].tobytes()                  # alone in time, batch and padding
        for b in range(rows):
            _close(f'V={V} steps={n_steps[b]} score', got['score'][b], score_hi[b], _bound(score_hi[b], score_lo[b], abs(score_hi[b])))
    assert outs[0][0]['score'][0] == 0 and outs[0][0]['n_out'][0] == 0


# ---- dx_edit_distance --------------------------------------------------------------------------------------------------------------------

def _edit(pairs, R, Hn):
    ''' `dx_edit_distance` on [(ref, hyp)] with the padded extents R, Hn: garbage behind the lengths, the output poisoned '''
    from daft_exprt import _hip as H
    B = len(pairs)
    ref, hyp = np.full((B, max(R, 1)), -123456, dtype=np.int32), np.full((B, max(Hn, 1)), 987654, dtype=np.int32)
    for b, (r, h) in enumerate(pairs):
        ref[b, :len(r)], hyp[b, :len(h)] = r, h
        ref[b, len(r):] = h[0] if len(h) else 5                              # garbage that would match if it were read
    n_ref, n_hyp = (np.array([len(p[k]) for p in pairs], dtype=np.int64) for k in (0, 1))
    counts = torch.full((B, 4), -77, dtype=torch.int32, device=DEV)
    rd, hd, nr, nh = (_dev(ref[:, :R]) if R else None), (_dev(hyp[:, :Hn]) if Hn else None), _dev(n_ref), _dev(n_hyp)
    H.check(H.lib().dx_edit_distance(H.ptr(rd), H.ptr(nr), H.ptr(hd), H.ptr(nh), H.ptr(counts), B, R, Hn, H.stream()))
    return counts.cpu().numpy()


def test_edit_distance_is_exact_batched_and_alone():
    from daft_exprt.recognizer import edit_distance, edit_max_len
    limit = edit_max_len()
    cases = O.edit_cases(limit)
    want = np.array([O.edit_counts_diagonals(r, h) for _, r, h in cases], dtype=np.int32)
    assert (want[:, 0] + want[:, 1] + want[:, 3] == [len(r) for _, r, _ in cases]).all()
    assert (want[:, 0] + want[:, 2] + want[:, 3] == [len(h) for _, _, h in cases]).all()
    batched = _edit([(r, h) for _, r, h in cases], limit, limit)
    for i, (name, r, h) in enumerate(cases):
        print(f'{name}: {len(r)} x {len(h)} -> sub, del, ins, match {batched[i].tolist()}')
        assert batched[i].tolist() == want[i].tolist(), name
        assert _edit([(r, h)], len(r), len(h))[0].tolist() == want[i].tolist(), name          # alone, tight extents (0 included)
    small = [(r, h) for _, r, h in cases if len(r) <= 70 and len(h) <= 70]
    for (r, h), got in zip(small, _edit(small, 70, 70)):                                       # the definition in plain loops
        assert got.tolist() == list(O.edit_counts(r.tolist(), h.tolist()))
    ref, hyp = torch.tensor([[1, 2, 3, 9]], dtype=torch.int32, device=DEV), torch.tensor([[1, 3, 9, 9]], dtype=torch.int32, device=DEV)
    assert edit_distance(ref, torch.tensor([3], device=DEV), hyp, torch.tensor([2], device=DEV)).tolist() == [[0, 1, 0, 2]]
    assert edit_distance(ref, torch.tensor([99], device=DEV), hyp, torch.tensor([-4], device=DEV)).tolist() == [[0, 4, 0, 0]]   # clamped
    with pytest.raises(ValueError, match='at most'):
        edit_distance(torch.zeros((1, limit + 1), dtype=torch.int32, device=DEV), torch.tensor([1], device=DEV), hyp, torch.tensor([1], device=DEV))


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------

def test_autograd_against_float64_ctc_loss_and_skipped_rows():
    ''' `uctc_loss` is `F.ctc_loss(..., reduction='mean')` over the rows with status 0: value and gradient against float64 autograd
        on the CPU, each row under the bound of its own fp32 restatement (the oracle run with the row's weight 1 / (labels x rows)) '''
    import torch.nn.functional as F
    from daft_exprt.recognizer import uctc_loss
    c = _case(65, 'short')
    ok = [b for b in range(c['B']) if c['status'][b] == 0]
    x = _dev(c['logits']).requires_grad_()
    args = [_dev(c[k]) for k in ('n_steps', 'labels', 'n_labels')]
    loss, skipped = uctc_loss(x, *args)
    loss.backward()
    assert int(skipped) == 3 and not x.grad[[7, 8, 9]].any()
    x64 = torch.tensor(c['logits'][ok], dtype=torch.float64, requires_grad=True)
    want = F.ctc_loss(F.log_softmax(x64, dim=2).transpose(0, 1), torch.tensor(c['labels'][ok]), torch.tensor(c['n_steps'][ok]),
                      torch.tensor(c['n_labels'][ok]), blank=0, reduction='mean')
    want.backward()
    w = 1.0 / (np.maximum(c['n_labels'], 1) * len(ok))
    per_hi, _, grad_hi = C.ctc_loss(c['logits'], c['n_steps'], c['labels'], c['n_labels'], w, np.float64)
    per_lo, _, grad_lo = C.ctc_loss(c['logits'], c['n_steps'], c['labels'], c['n_labels'], w, np.float32)
    assert abs(float(want) - float((per_hi[ok] * w[ok]).sum())) < 1e-9 * abs(float(want))          # the oracle is torch's mean
    bound = sum(_bound(per_hi[b], per_lo[b], max(abs(per_hi[b]), float(np.abs(c['logits'][b, :c['n_steps'][b]]).max()))) * w[b] for b in ok)
    _close('mean loss', float(loss.detach()), float(want), bound + 4 * EPS * abs(float(want)))
    got = x.grad.cpu().numpy()
    for i, b in enumerate(ok):
        nT = int(c['n_steps'][b])
        assert np.abs(grad_hi[b, :nT] - x64.grad[i, :nT].numpy()).max() < 1e-9
        largest = float(np.abs(c['logits'][b, :nT]).max())
        _close(f'row {b} grad', got[b, :nT], x64.grad[i, :nT].numpy(), _bound(grad_hi[b, :nT], grad_lo[b, :nT], largest * w[b]))
        assert not got[b, nT:].any()


# ---- learnability ------------------------------------------------------------------------------------------------------------------------

RESTATEMENT = (0.0382, 0.0350, 0.0541, 0.0446, 0.0478, 0.0382)      # tests/recognizer_oracle.py toy_restatement(seed), seeds 0 .. 5
CEILING = max(RESTATEMENT) + (max(RESTATEMENT) - min(RESTATEMENT))  # their maximum plus their spread: 0.0732


def _errors(model, utts, text):
    ''' the summed sub + del + ins of `phone_error_rates` of the fabricated `utts` against the phones of `text`, and their count '''
    from daft_exprt.recognizer import phone_error_rates
    _, _, mel, nt = (t.to(DEV) for t in O.toy_collate(utts, torch.float32))
    sym, nl, _, _ = (t.to(DEV) for t in O.toy_collate(text, torch.float32))
    s = phone_error_rates(model, mel, nt, sym, nl)
    assert int((s['n_ref'].long() - nl).abs().sum()) == 0                    # every toy symbol is a phone
    return int(s['sub'].sum() + s['del'].sum() + s['ins'].sum()), int(s['n_ref'].sum())


@functools.lru_cache(maxsize=None)
def _trained():
    ''' (the toy recogniser after training, its held-out error count before, the rows skipped), trained once for both tests '''
    from daft_exprt.recognizer import Recognizer, uctc_loss
    cfg = O.TOY
    train, held = O.toy_split(O.toy_corpus())
    sym, nl, mel, nt = (t.to(DEV) for t in O.toy_collate(train, torch.float32))
    seed = 0
    torch.manual_seed(seed)
    model = Recognizer(O.TOY_SYMBOLS, cfg['n_mel'], hidden=cfg['hidden'], layers=cfg['layers'], stride=cfg['stride']).to(DEV)
    before = _errors(model, held, held)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=cfg['lr'])
    skipped_rows = torch.zeros((), dtype=torch.int64, device=DEV)
    for idx in O.toy_batches(seed, len(train)):
        idx = torch.tensor(idx, device=DEV)
        labels, n_labels = model.labels_of(sym[idx], nl[idx])
        logits, n_steps = model(mel[idx], nt[idx])
        loss, skipped = uctc_loss(logits, n_steps, labels, n_labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        skipped_rows += skipped
    model.eval()
    return model, before, int(skipped_rows), float(loss.detach())


def test_the_recognizer_learns_the_toy_corpus():
    ''' 200 fabricated utterances of 4 to 12 phones over 15 classes, 2 to 7 frames per phone, each frame its phone's fixed random
        template plus 0.3 x Gaussian noise; 160 train Recognizer(hidden 64, 2 convolutions, stride 2) for 400 Adam steps at 3e-3
        with 32 utterances each, the other 40 are scored with `phone_error_rates`.  The held-out phone error rate must not exceed
        the ceiling 0.0732 = the maximum plus the spread (max - min) of `recognizer_oracle.toy_restatement` -- plain torch,
        float64, CPU, `F.ctc_loss`, the same architecture, data and schedule -- which gave 0.0382, 0.0350, 0.0541, 0.0446,
        0.0478, 0.0382 for the seeds 0 .. 5 (untrained: 0.89 to 1.18). '''
    model, (errors_before, n_ref), skipped, loss = _trained()
    held = O.toy_split(O.toy_corpus())[1]
    errors, n = _errors(model, held, held)
    before, after = errors_before / n_ref, errors / n
    print(f'held-out phone error rate: untrained {before:.4f}, trained {after:.4f} ({errors} errors of {n} phones, loss {loss:.5f}); '
          f'ceiling {CEILING:.4f}')
    assert skipped == 0                                                      # 2 frames per phone at least, 2 frames per step
    assert before > 0.5
    assert after <= CEILING


@pytest.mark.parametrize('kind', ('delete', 'replace'))
def test_the_rate_measures_the_edits_made(kind):
    ''' the held-out utterances are fabricated again with ONE known phone deleted, or replaced by another, and scored against the
        unedited text: the errors beyond the clean count must be the number of edits made (40), to within the model's own clean
        error count '''
    model, _, _, _ = _trained()
    held = O.toy_split(O.toy_corpus())[1]
    clean, _ = _errors(model, held, held)
    edited, _ = _errors(model, O.toy_edits(held, kind), held)
    print(f'{kind}: {clean} errors on the clean utterances, {edited} on the edited ones: {edited - clean} extra for {len(held)} edits')
    assert abs((edited - clean) - len(held)) <= clean


# ---- the command lines, end to end -------------------------------------------------------------------------------------------------------

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


def _check_per(entry):
    from daft_exprt.recognizer import PER_KEYS
    assert tuple(entry) == PER_KEYS and all(isinstance(entry[k], int) and entry[k] >= 0 for k in ('sub', 'del', 'ins', 'n_ref', 'n_hyp'))
    assert entry['n_ref'] > 0 and np.isfinite(entry['per'])
    assert entry['sub'] + entry['del'] + entry['ins'] == round(entry['per'] * entry['n_ref'])
    assert entry['n_hyp'] - entry['ins'] == entry['n_ref'] - entry['del']


def _checkpoint_and_recognizer(golden_dir, tmp_path, steps):
    ''' a tiny acoustic model's checkpoint, the file list of tests/golden and a recogniser `train_recognizer.py` trained on it '''
    from tests.test_gpu_dtw import _file_list, _tiny_model
    model, hp = _tiny_model(golden_dir)
    ckpt = str(tmp_path / 'DaftExprt_test')
    torch.save({'iteration': 0, 'state_dict': {f'module.{k}': v for k, v in model.state_dict().items()}, 'config_params': dict(vars(hp))}, ckpt)
    list_file, names, _ = _file_list(golden_dir, tmp_path)
    rec_path = str(tmp_path / 'recognizer.pt')
    report = _cli('train_recognizer').main(['-chk', ckpt, '-tf', list_file, '-vf', list_file, '-o', rec_path, '-st', str(steps), '-bs', '4',
                                            '-hid', '32', '-ly', '2', '--seed', '3'])
    return hp, ckpt, list_file, names, rec_path, report


def test_train_recognizer_then_evaluate_with_it(golden_dir, tmp_path):
    from daft_exprt.evaluate import PER_LEVELS
    from daft_exprt.recognizer import PER_KEYS, Recognizer, load_recognizer
    hp, ckpt, list_file, names, rec_path, returned = _checkpoint_and_recognizer(golden_dir, tmp_path, 30)
    report = json.load(open(tmp_path / 'recognizer_report.json'))
    assert json.loads(json.dumps(returned)) == report
    assert report['utterances_train'] + report['left_out'] == 5 == report['utterances_held_out'] and report['skipped_rows'] == 0
    assert report['steps'] == 30 and np.isfinite(report['loss']) and len(report['held_out_decodes']) == 5
    assert 0 <= report['phone_error_rate_folded'] <= report['phone_error_rate'] and report['errors']['n_ref'] > 0
    assert report['phone_error_rate'] == sum(report['errors'][k] for k in ('sub', 'del', 'ins')) / report['errors']['n_ref']
    rec = load_recognizer(rec_path)
    assert isinstance(rec, Recognizer) and all(p.is_cuda and torch.isfinite(p).all() for p in rec.parameters()) and rec.args['hidden'] == 32
    plain, scored = str(tmp_path / 'plain'), str(tmp_path / 'scored')
    evaluate = _cli('evaluate')
    evaluate.main(['-chk', ckpt, '-vf', list_file, '-out', plain])
    evaluate.main(['-chk', ckpt, '-vf', list_file, '-out', scored, '-rec', rec_path])
    a, b = (json.load(open(os.path.join(d, 'copy_synthesis.json'))) for d in (plain, scored))
    assert list(a) == ['audio', 'files', 'summary'] and all(list(e) == ['speaker_id', 'mel', 'audio'] for e in a['files'].values())
    assert list(a['summary']) == ['files', 'mel', 'audio', 'speakers'] and all(list(s) == ['files', 'mel', 'audio'] for s in a['summary']['speakers'].values())
    for name in names:                                                       # -rec adds `per` and changes nothing else
        entry = dict(b['files'][name])
        per = entry.pop('per')
        assert entry == a['files'][name] and tuple(per) == PER_LEVELS
        for level in PER_LEVELS:
            _check_per(per[level])
        assert per['recording']['n_ref'] == per['mel']['n_ref'] == per['audio']['n_ref']
    for table in [b['summary']] + list(b['summary']['speakers'].values()):
        assert tuple(table['per']) == PER_LEVELS
        for level in PER_LEVELS:
            assert set(table['per'][level]) == set(PER_KEYS) | {'rate'} and np.isfinite(table['per'][level]['rate'])
            assert table['per'][level]['per']['count'] == table['files']
    stripped = json.loads(json.dumps(b['summary']))
    for table in [stripped] + list(stripped['speakers'].values()):
        del table['per']
    assert stripped == a['summary']
    want = sum(b['files'][n]['per']['audio'][k] for n in names for k in ('sub', 'del', 'ins')) / sum(b['files'][n]['per']['audio']['n_ref'] for n in names)
    assert b['summary']['per']['audio']['rate'] == pytest.approx(want)


def test_synthesize_with_a_recognizer_writes_intelligibility(golden_dir, tmp_path):
    ''' `scripts/synthesize.py -rec R` (a script that takes its arguments from the command line only: two child processes) '''
    from tests.test_gpu_prosody_eval import _style_bank
    hp, ckpt, _, _, rec_path, _ = _checkpoint_and_recognizer(golden_dir, tmp_path, 3)
    bank = str(tmp_path / 'bank')
    _style_bank(bank, hp)
    text = tmp_path / 'sentences_to_generate.txt'
    text.write_text('s.txt_line0|{HH AH0 L OW1} {W ER1 L D} , {T EH1 S T} ? ~\ns.txt_line1|{T EH1 S T} . ~\n', encoding='utf-8')
    outs = []
    for out_dir, extra in ((str(tmp_path / 'syn_plain'), ()), (str(tmp_path / 'syn_scored'), ('-rec', rec_path))):
        _script('synthesize', '-out', out_dir, '-chk', ckpt, '-tf', str(text), '-sb', bank, '-bs', '2', *extra)
        outs.append(out_dir)
    assert not os.path.exists(os.path.join(outs[0], 'intelligibility.json'))
    a, b = (json.load(open(os.path.join(d, 'prosody_transfer.json'))) for d in outs)
    assert a == b                                                            # the same seed, the same audio, the same report
    report = json.load(open(os.path.join(outs[1], 'intelligibility.json')))
    assert list(report) == ['audio', 'files', 'summary'] and report['audio'] == 'griffin-lim' and sorted(report['files']) == sorted(b['files'])
    for name, entry in report['files'].items():
        assert entry.pop('wav') == b['files'][name]['wav'] and os.path.isfile(os.path.join(outs[1], b['files'][name]['wav']))
        _check_per(entry)
    assert sorted(e['n_ref'] for e in report['files'].values()) == [4, 12]   # the phones of the two sentences, nothing else
    s = report['summary']
    assert s['files'] == 2 and s['n_ref'] == 16 and s['rate'] == (s['sub'] + s['del'] + s['ins']) / 16
