"""K30 (csrc/g2p.hip) and daft_exprt/g2p.py on the GPU against tests/ctc_oracle.py.

The float outputs are compared with the float64 oracle on the same (fp32-representable) inputs.  The bound is measured, not
assumed: the float32 restatement of the same recurrence runs on the same inputs on the CPU, and the kernel is allowed 4 x its
largest deviation from float64 (the kernel's butterflies add in another order), with a floor of 8 fp32 ulps of the larger of 1,
|loss| and the largest |logit| for the loss, and of the larger of 1 and |w| x the largest |logit| for the gradient -- see
`_bound`.  The greedy decode is an integer result and must equal the oracle exactly.  Every launch gets its dead inputs as NaN /
garbage and its outputs and workspace pre-filled with NaN / garbage, and every word is run in the ragged batch, in a batch
with larger padded extents, and alone: the three must agree bit for bit."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ctc_oracle as O
from tests.util import make_hparams

DEV = 'cuda:0'
EPS = float(np.finfo(np.float32).eps)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bound(hi, lo, scale):
    ''' max(4 x the largest deviation of the float32 restatement `lo` from the float64 oracle `hi`, 8 eps32 x max(1, scale)).
        For the loss `scale` is the larger of |loss| of the word and its largest |logit|: a log-probability x - z is a difference
        of two numbers of the logits' magnitude, each rounded to half an ulp of it, and the loss is a sum of n_steps of them and
        carries a few half-ulps of its own magnitude however the sums are ordered.  For the gradient `scale` is |w| times the
        largest |logit|: an entry is w (softmax - posterior), both at most 1, and the softmax exp(x - z) inherits the rounding
        of x - z; what the length of the word adds to the posteriors is not in the floor -- the measured deviation carries it.
        The floor keeps words whose restatement happens to round exactly (one step, one label) from demanding more than the
        format holds. '''
    d = np.abs(np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64))
    return max(4.0 * float(d.max()) if d.size else 0.0, 8.0 * EPS * max(1.0, float(scale)))


def _close(name, got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.isfinite(got).all(), name
    err = float(np.abs(got - want).max()) if want.size else 0.0
    print(f'{name}: max error {err:.3e}, bound {tol:.3e}')
    assert err <= tol, (name, err, tol)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(V):
    ''' the ragged batch of `ctc_oracle.gpu_case`, the float64 oracle and the float32 restatement, computed once '''
    c = O.gpu_case(V)
    for tag, dt in (('hi', np.float64), ('lo', np.float32)):
        c['loss_' + tag], status, c['grad_' + tag] = O.ctc_loss(c['logits'], c['n_steps'], c['labels'], c['n_labels'], c['w'], dt)
        assert status.tolist() == c['status'].tolist()
    return c


def _run(c, rows=None, pad=(0, 0, 0)):
    ''' `dx_ctc_loss` on the words `rows` of a case (all by default) with the tight extents plus `pad` = (T, U, B): logits at or past
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
    ws = torch.full((B, T, 2 * U + 1), float('nan'), device=DEV)
    H.check(H.lib().dx_ctc_loss(H.ptr(x), H.ptr(nT), H.ptr(lab), H.ptr(nL), H.ptr(w), H.ptr(o['loss']), H.ptr(o['status']),
                                H.ptr(o['grad']), H.ptr(ws), B, T, U, V, H.stream()))
    return {name: t.cpu().numpy() for name, t in o.items()}


def _word(out, i, nT):
    ''' the bytes of word i of an output of `_run`, after checking that its steps at or past n_steps are +0 '''
    g = out['grad'][i]
    assert not g[nT:].any() and not np.signbit(g[nT:]).any()
    return out['loss'][i].tobytes() + out['status'][i].tobytes() + g[:nT].tobytes()


@pytest.mark.parametrize('V', O.CLASSES)
def test_loss_and_gradient_against_float64_alone_in_a_batch_and_padded(V):
    ''' Measured on the CPU (float32 restatement against float64, the same inputs): the largest deviation over the words of the
        case, at the word where it occurs, and the bound that word gets (4 x the deviation; the floor decides the short words):
          V = 2:    loss 1.5e-04 -> bound 5.9e-04 (256 x 127),  gradient 1.6e-04 -> 6.5e-04 (256 x 127)
          V = 29:   loss 2.3e-04 -> bound 9.3e-04 (192 x 64),   gradient 6.6e-04 -> 2.6e-03 (192 x 64)
          V = 77:   loss 1.0e-04 -> bound 1.1e-03 (256 x 127, the floor at |loss| 1.2e+03),  gradient 2.2e-04 -> 8.9e-04 (256 x 127)
          V = 128:  loss 1.3e-04 -> bound 9.2e-04 (192 x 64),   gradient 8.8e-04 -> 3.5e-03 (256 x 127)
        and for the words of at most 5 steps deviations of 1e-08 to 3e-06 against bounds of 1e-06 to 3e-05 (the floor).  The test
        prints every word's own figures. '''
    c = _case(V)
    shapes = O.SHAPES + O.DEAD
    batch, again = _run(c), _run(c)
    for name in batch:                                                       # two runs: bit-equal
        assert batch[name].tobytes() == again[name].tobytes(), name
    assert batch['status'].tolist() == c['status'].tolist()
    inner = [b for b, (nT, nL) in enumerate(shapes) if nT + 3 <= 256 and nL + 5 <= 127]
    wide = _run(c, rows=inner, pad=(3, 5, 2))                                # every extent larger: T, U (another K), B
    assert wide['status'][len(inner):].tolist() == [2, 2] and np.isnan(wide['loss'][len(inner):]).all()
    assert not wide['grad'][len(inner):].any()
    for b, (nT, nL) in enumerate(shapes):
        alone = _run(c, rows=[b])
        assert _word(batch, b, nT) == _word(alone, 0, nT), (V, nT, nL)
        if b in inner:
            assert _word(batch, b, nT) == _word(wide, inner.index(b), nT), (V, nT, nL)
        tag = f'V={V} {nT}x{nL} '
        if c['status'][b] != 0:
            assert np.isnan(batch['loss'][b]) and not batch['grad'][b].any()
            continue
        hi, lo, w = c['loss_hi'][b], c['loss_lo'][b], float(c['w'][b])
        largest = float(np.abs(c['logits'][b, :nT]).max())
        _close(tag + 'loss', batch['loss'][b], hi, _bound(hi, lo, max(abs(hi), largest)))
        _close(tag + 'grad', batch['grad'][b, :nT], c['grad_hi'][b, :nT],
               _bound(c['grad_hi'][b, :nT], c['grad_lo'][b, :nT], largest * w))
        assert not batch['grad'][b, nT:].any()


def test_a_label_out_of_range_is_a_status_not_a_fault():
    from daft_exprt.g2p import ctc_loss_and_grad
    x = torch.zeros((3, 4, 5), device=DEV)
    labels = torch.tensor([[1, 5], [0, 1], [4, 4]], device=DEV)
    loss, status, grad = ctc_loss_and_grad(x, torch.tensor([4, 4, 4], device=DEV), labels, torch.tensor([2, 1, 2], device=DEV))
    assert status.tolist() == [3, 3, 0] and torch.isnan(loss[:2]).all() and not grad[:2].any() and torch.isfinite(loss[2])
    with pytest.raises(ValueError, match='at most'):
        ctc_loss_and_grad(torch.zeros((1, 257, 5), device=DEV), torch.tensor([4], device=DEV), labels[:1], torch.tensor([2], device=DEV))


# ---- greedy decoding ----------------------------------------------------------------------------------------------------------------------

GREEDY_STEPS = (0, 1, 2, 5, 9, 64, 65, 200, 256)


def _greedy_case(V, seed=5):
    ''' logits on a grid of multiples of 1/8 drawn from few values, so ties abound; word 4 is written by hand: the path
        1 1 0 1 V-1 V-1 0 0 1 collapses to 1 1 V-1 1 (a repeat across a blank stays two, a repeat without one collapses) '''
    rng = np.random.RandomState(seed + V)
    B, T = len(GREEDY_STEPS), max(GREEDY_STEPS)
    x = (rng.randint(0, 4, size=(B, T, V)) * rng.choice([0.125, 0.5, 1.0], size=(B, T, 1))).astype(np.float32)
    x[4, :9] = -1.0
    for t, cls in enumerate([1, 1, 0, 1, V - 1, V - 1, 0, 0, 1]):
        x[4, t, cls] = 0.5
    return x, np.array(GREEDY_STEPS, dtype=np.int64)


@pytest.mark.parametrize('V', O.CLASSES)
def test_greedy_decode_is_exact(V):
    from daft_exprt import _hip as H
    x, n_steps = _greedy_case(V)
    B, T = x.shape[:2]
    want_ids, want_n, score_hi = O.greedy(x, n_steps)
    score_lo = O.greedy(x, n_steps, np.float32)[2]
    assert want_ids[4, :want_n[4]].tolist() == ([1, 1, V - 1, 1] if V > 2 else [1, 1, 1])      # (V = 2: class V - 1 is class 1)
    ties = sum(int((np.sort(x[b, :n], axis=1)[:, -1] == np.sort(x[b, :n], axis=1)[:, -2]).sum()) for b, n in enumerate(n_steps))
    assert ties > 20
    outs = []
    for pad in (0, 0, 7):
        Tp = min(T + pad, 256)
        xp = np.full((B + (pad > 0), Tp, V), np.nan, dtype=np.float32)
        nT = np.zeros((B + (pad > 0),), dtype=np.int64)
        nT[:B] = n_steps
        for b, n in enumerate(n_steps):
            xp[b, :n] = x[b, :n]
        o = dict(ids=torch.full(xp.shape[:2], -77, dtype=torch.int32, device=DEV), n_out=torch.full((len(nT),), -77, dtype=torch.int32, device=DEV),
                 score=torch.full((len(nT),), float('nan'), device=DEV))
        H.check(H.lib().dx_ctc_greedy(H.ptr(_dev(xp)), H.ptr(_dev(nT)), H.ptr(o['ids']), H.ptr(o['n_out']), H.ptr(o['score']), len(nT), Tp, V,
                                      H.stream()))
        outs.append({k: v.cpu().numpy() for k, v in o.items()})
    for got in outs:
        assert got['n_out'][:B].tolist() == want_n.tolist()
        assert np.array_equal(got['ids'][:B, :T], want_ids) and not got['ids'][:B, T:].any()       # zero-filled behind n_out
        assert got['score'][:B].tobytes() == outs[0]['score'].tobytes()
        for b in range(B):
            _close(f'V={V} steps={n_steps[b]} score', got['score'][b], score_hi[b], _bound(score_hi[b], score_lo[b], abs(score_hi[b])))
    assert outs[0]['score'][0] == 0 and outs[0]['n_out'][0] == 0


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------

def test_autograd_and_skipped_rows():
    from daft_exprt.g2p import ctc_loss, ctc_loss_and_grad
    c = _case(29)
    x = _dev(c['logits']).requires_grad_()
    args = [_dev(c[k]) for k in ('n_steps', 'labels', 'n_labels')]
    loss, skipped = ctc_loss(x, args[0], args[1], args[2])
    (3.0 * loss).backward()
    per, status, grad = ctc_loss_and_grad(x.detach(), args[0], args[1], args[2])
    ok = status == 0
    assert int(skipped) == 2 and int(ok.sum()) == len(O.SHAPES)
    up = torch.where(ok, torch.full_like(per, 3.0 / len(O.SHAPES)), torch.zeros_like(per))
    assert torch.allclose(x.grad, grad * up[:, None, None], rtol=1e-6, atol=0) and not x.grad[~ok].any()
    keep = torch.nonzero(ok)[:, 0]
    only, none = ctc_loss(x.detach()[keep], args[0][keep], args[1][keep], args[2][keep])
    loss = float(loss.detach())
    assert int(none) == 0 and abs(float(only) - loss) <= 4 * EPS * abs(loss)                           # skipped rows do not move the mean
    want = float(np.mean(c['loss_hi'][:len(O.SHAPES)]))
    assert abs(loss - want) <= max(_bound(c['loss_hi'][b], c['loss_lo'][b], abs(c['loss_hi'][b])) for b in range(len(O.SHAPES)))


# ---- learnability ------------------------------------------------------------------------------------------------------------------------

RESTATEMENT = (0.0063, 0.0095, 0.0083, 0.0099, 0.0075, 0.0118)      # tests/ctc_oracle.py toy_restatement(seed), seeds 0 .. 5
CEILING = max(RESTATEMENT) + 0.03


def test_the_g2p_learns_the_toy_lexicon():
    ''' 2 000 spellings of 2 to 10 letters over 12 letters, pronounced by the context rules of `ctc_oracle.toy_pronounce`; 1 600
        train G2P(hidden 64, 3 slots per letter) for 400 Adam steps at 4e-3 with 64 words each, the other 400 are decoded.  The
        held-out phone error rate must not exceed max(restatement) + 0.03 = 0.0418, the restatement being
        `ctc_oracle.toy_restatement` -- plain torch, float64, CPU, `F.ctc_loss`, the same architecture, data and schedule -- which
        gave 0.0063, 0.0095, 0.0083, 0.0099, 0.0075, 0.0118 for the seeds 0 .. 5 (untrained: 1.1 to 2.1). '''
    from daft_exprt.g2p import G2P, ctc_loss
    cfg = O.TOY
    train, held = O.toy_split(O.toy_lexicon())
    g, n, lab, nl = (t.to(DEV) for t in O.toy_pack(train))
    seed = 0
    torch.manual_seed(seed)
    model = G2P(O.TOY_PHONES, hidden=cfg['hidden'], expand=cfg['expand']).to(DEV)

    def rate():
        return O.phone_error_rate(model.phonemize([w for w, _ in held]), [p for _, p in held])

    before = rate()
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=cfg['lr'])
    skipped_rows = torch.zeros((), dtype=torch.int64, device=DEV)
    for idx in O.toy_batches(seed, len(train)):
        idx = torch.tensor(idx, device=DEV)
        logits, n_steps = model(g[idx], n[idx])
        loss, skipped = ctc_loss(logits, n_steps, lab[idx], nl[idx])
        opt.zero_grad()
        loss.backward()
        opt.step()
        skipped_rows += skipped
    after = rate()
    print(f'held-out phone error rate: untrained {before:.4f}, trained {after:.4f} (loss {float(loss.detach()):.5f}); ceiling {CEILING:.4f}')
    assert int(skipped_rows) == 0                                           # with 3 slots per letter every toy word has a path
    assert before > 0.5
    assert after <= CEILING


# ---- the command lines, end to end -------------------------------------------------------------------------------------------------------

def _cli(name):
    spec = importlib.util.spec_from_file_location(f'{name}_cli', os.path.join(ROOT, 'scripts', f'{name}.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_train_g2p_then_phonemize(tmp_path):
    from daft_exprt.g2p import G2P, load_g2p
    from daft_exprt.generate import _symbol_ids, read_phonemised_sentences
    hp = make_hparams()
    lexicon = O.toy_lexicon(seed=7, words=340)                              # the toy phones are ARPAbet phones of the symbol table
    listed, unlisted = lexicon[:300], [w for w, _ in lexicon[300:]]
    dictionary = tmp_path / 'toy.dict'
    dictionary.write_text(''.join(f'{w} {" ".join(p)}\n' for w, p in listed) + f'{listed[0][0]}(2) {" ".join(listed[1][1])}\n', encoding='utf-8')
    report = _cli('train_g2p').main(['-dict', str(dictionary), '-o', str(tmp_path / 'g2p.pt'), '-st', '300', '-bs', '64', '-hid', '32',
                                     '-lr', '4e-3', '--seed', '3'])
    with open(tmp_path / 'g2p_report.json', 'r', encoding='utf-8') as f:
        written = json.load(f)
    assert written['words_train'] == 285 and written['words_held_out'] == 15 and written['skipped_rows'] == 0 == report['skipped_rows']
    assert 0 <= written['phone_error_rate'] and 0 <= written['word_error_rate'] <= 1 and len(written['held_out_decodes']) == 15
    g2p = load_g2p(str(tmp_path / 'g2p.pt'))
    assert isinstance(g2p, G2P) and all(p.is_cuda and torch.isfinite(p).all() for p in g2p.parameters()) and g2p.args['hidden'] == 32
    assert g2p.phonemize(['b2b', '', unlisted[0]])[:2] == [None, None]     # a character outside the table; no character at all

    a, b, c, d = (w for w, _ in listed[:4])
    text = tmp_path / 'corpus.txt'
    text.write_text(f'{a.capitalize()} {unlisted[0]}, {b} -- {c}!\nutt_b|{unlisted[1]} {d}? {unlisted[0]} {unlisted[2]}.\n{c} {d}\n', encoding='utf-8')
    out = tmp_path / 'out'
    summary = _cli('phonemize').main(['-tf', str(text), '-dict', str(dictionary), '-g2p', str(tmp_path / 'g2p.pt'), '-out', str(out)])
    with open(out / 'phonemize_report.json', 'r', encoding='utf-8') as f:
        written = json.load(f)
    assert written == summary and sorted(written['oov']) == sorted(unlisted[:3]) and written['dictionary_words'] == 6
    assert all(p and set(p.split()) <= set(O.TOY_PHONES) for p in written['oov'].values())
    sentences, names = read_phonemised_sentences(str(out / 'sentences_to_generate.txt'), hp.symbols)
    assert names == ['corpus.txt_line0', 'utt_b', 'corpus.txt_line2'] and len(sentences) == 3
    assert [item for item in sentences[0] if not isinstance(item, list)] == [' ', ',', ',', '!', '~']
    assert sentences[2] == [listed[2][1], ' ', listed[3][1], '~']
    for sentence in sentences:
        ids = _symbol_ids(sentence, hp)
        assert ids and all(0 < i < len(hp.symbols) for i in ids)
    # without the model the same file is an error that names the words
    with pytest.raises(ValueError, match=unlisted[0]):
        _cli('phonemize').main(['-tf', str(text), '-dict', str(dictionary), '-out', str(tmp_path / 'out2')])


def test_synthesize_from_raw_text(golden_dir, tmp_path):
    ''' `scripts/synthesize.py -dict D -g2p G` on plain lines: phonemised first, then audio, with no other program involved '''
    import subprocess
    import sys
    from daft_exprt.g2p import G2P, save_g2p
    from daft_exprt.generate import read_phonemised_sentences
    from tests.test_gpu_prosody_eval import _style_bank, _tiny_model
    model, hp = _tiny_model(golden_dir)
    ckpt = str(tmp_path / 'DaftExprt_test')
    torch.save({'iteration': 0, 'state_dict': {f'module.{k}': v for k, v in model.state_dict().items()}, 'config_params': dict(vars(hp))}, ckpt)
    bank, out_dir = str(tmp_path / 'bank'), str(tmp_path / 'out')
    _style_bank(bank, hp)
    dictionary = tmp_path / 'small.dict'
    dictionary.write_text('hello HH AH0 L OW1\nworld W ER1 L D\n', encoding='utf-8')
    torch.manual_seed(5)
    g2p = G2P(O.TOY_PHONES, hidden=16)
    with torch.no_grad():
        g2p.out.bias[0] = -20.0                                             # untrained, but never the blank: every word decodes to something
    save_g2p(g2p, str(tmp_path / 'g2p.pt'))
    text = tmp_path / 'lines.txt'
    text.write_text('Hello, world!\nHello zog.\n', encoding='utf-8')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'synthesize.py'), '-out', out_dir, '-chk', ckpt, '-tf', str(text), '-sb', bank,
                        '-bs', '2', '-dict', str(dictionary), '-g2p', str(tmp_path / 'g2p.pt')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'not in the dictionary: "zog"' in r.stderr
    sentences, names = read_phonemised_sentences(os.path.join(out_dir, 'sentences_to_generate.txt'), hp.symbols)
    assert names == ['lines.txt_line0', 'lines.txt_line1'] and sentences[0] == [['HH', 'AH0', 'L', 'OW1'], ',', ['W', 'ER1', 'L', 'D'], '!', '~']
    assert sentences[1][0] == ['HH', 'AH0', 'L', 'OW1'] and sentences[1][1] == ' ' and set(sentences[1][2]) <= set(O.TOY_PHONES)
    report = json.load(open(os.path.join(out_dir, 'prosody_transfer.json')))
    wavs = [f for f in os.listdir(out_dir) if f.endswith('.wav') and '_ref.wav' not in f]
    assert len(report['files']) == 2 and len(wavs) == 2 and all(os.path.getsize(os.path.join(out_dir, f)) > 1000 for f in wavs)
