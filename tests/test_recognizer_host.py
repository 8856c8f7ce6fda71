"""The host side of the intelligibility score, without a GPU: tests/recognizer_oracle.py's edit distance is pinned
against an enumeration of all alignments and against `ctc_oracle.edit_distance`; the host logic of daft_exprt/recognizer.py (label
mapping, stress folding, the step count, the masks of the encoder) on CPU tensors; the limits and symbols of K31 through the ABI."""
import itertools

import numpy as np
import pytest
import torch

from tests import ctc_oracle as C
from tests import recognizer_oracle as O
from tests.util import make_hparams


# ---- the edit oracle ---------------------------------------------------------------------------------------------------------------------

def _restricted_growth(n, k):
    ''' the sequences of length n over 1 .. k whose symbols first appear in the order 1, 2, ...: one per renaming class '''
    return [s for s in itertools.product(range(1, k + 1), repeat=n) if all(c <= max((0,) + s[:i]) + 1 for i, c in enumerate(s))]


def test_edit_oracle_against_all_alignments():
    ''' every pair of sequences of at most 4 entries over 3 symbols -- the reference up to a renaming of the symbols, which changes
        no comparison -- : the cost is the minimum over ALL alignments, and the counts are those of the first cheapest alignment
        under the stated preference (diagonal, deletion, insertion, decided from the last move backwards) '''
    pairs = ties = 0
    for R, H in itertools.product(range(5), repeat=2):
        for ref in _restricted_growth(R, 3):
            for hyp in itertools.product(range(1, 4), repeat=H):
                cost, counts = O.first_cheapest(ref, hyp)
                got = O.edit_counts(ref, hyp)
                assert sum(got[:3]) == cost and got == counts, (ref, hyp, got, counts)
                assert got[0] + got[1] + got[3] == R and got[0] + got[2] + got[3] == H
                assert got == O.edit_counts_diagonals(ref, hyp)
                pairs += 1
                ties += len({a[2] for a in O.enumerate_alignments(ref, hyp) if a[0] == cost}) > 1
    assert pairs == 23 * 121 and ties > 300                     # the preference decides many of them


def test_edit_oracle_totals_and_the_diagonal_walk():
    rng = np.random.RandomState(3)
    for R, H, k in ((0, 0, 2), (0, 5, 2), (5, 0, 2), (1, 1, 2), (63, 65, 2), (64, 64, 3), (65, 63, 12), (40, 90, 2), (120, 100, 30)):
        ref, hyp = rng.randint(1, k + 1, size=R), rng.randint(1, k + 1, size=H)
        got = O.edit_counts(ref.tolist(), hyp.tolist())
        assert sum(got[:3]) == C.edit_distance(ref.tolist(), hyp.tolist()), (R, H, k)
        assert got == O.edit_counts_diagonals(ref, hyp), (R, H, k)
    assert O.edit_counts([1, 2, 3], [1, 2, 3]) == (0, 0, 0, 3) and O.edit_counts([1, 2], [3, 4]) == (2, 0, 0, 0)
    assert O.edit_counts([1, 2, 3], [1, 3]) == (0, 1, 0, 2) and O.edit_counts([1, 3], [1, 2, 3]) == (0, 0, 1, 2)
    # a tie: [1, 1] against [1] is one deletion either way; the diagonal is preferred at the last cell, so the FIRST entry is deleted
    assert O.edit_counts([1, 1], [1]) == (0, 1, 0, 1)
    for name, ref, hyp in O.edit_cases(300):
        assert len(ref) <= 300 and len(hyp) <= 300


def test_toy_corpus_and_edits():
    utts = O.toy_corpus()
    assert len(utts) == O.TOY['utterances'] and all(4 <= len(u[0]) <= 12 and int(u[1].min()) >= 2 and int(u[1].max()) <= 7 for u in utts)
    assert all((u[0][1:] != u[0][:-1]).all() and u[2].shape == (int(u[1].sum()), O.TOY['n_mel']) for u in utts)
    assert all((int(u[1].sum()) + 1) // 2 >= len(u[0]) for u in utts)                          # a CTC path at stride 2
    train, held = O.toy_split(utts)
    assert len(train) == 160 and len(held) == 40
    for kind in ('delete', 'replace'):
        edited = O.toy_edits(held, kind)
        for (cls, dur, noise), (ecls, edur, enoise) in zip(held, edited):
            assert (ecls[1:] != ecls[:-1]).all() and enoise.shape[0] == int(edur.sum())
            want = (0, 1, 0, len(cls) - 1) if kind == 'delete' else (1, 0, 0, len(cls) - 1)
            assert O.edit_counts(cls.tolist(), ecls.tolist()) == want
    sym, nl, mel, nt = O.toy_collate(held[:3], torch.float64)
    assert sym.min() == 0 and int(sym[sym > 0].min()) >= O.TOY_FIRST and mel.shape[1] == O.TOY['n_mel'] and int(nt.max()) == mel.shape[2]


# ---- the host logic of the model ---------------------------------------------------------------------------------------------------------

def test_labels_of_and_stress_fold():
    from daft_exprt.g2p import phones_of
    from daft_exprt.recognizer import Recognizer, stress_fold
    hp = make_hparams()
    rec = Recognizer(hp.symbols, 8, hidden=8, layers=1)
    phones = phones_of(hp.symbols)
    assert rec.phones == phones and rec.out.out_features == 1 + len(phones) and len(phones) == 69
    ids = lambda seq: [hp.symbols.index(s) for s in seq]
    a = ids(['HH', 'AH0', ' ', 'L', 'OW1', ',', 'AH1', '.', '~'])
    b = ids([' ', 'T', '~'])
    sym = torch.zeros((3, 9), dtype=torch.int64)
    sym[0, :9], sym[1, :3] = torch.tensor(a), torch.tensor(b)
    sym[1, 3:] = hp.symbols.index('S')                                                  # garbage behind the length
    labels, n = rec.labels_of(sym, torch.tensor([9, 3, 0]))
    assert n.tolist() == [5, 1, 0] and labels.shape == (3, 9)
    assert [phones[c - 1] for c in labels[0, :5].tolist()] == ['HH', 'AH0', 'L', 'OW1', 'AH1'] and not labels[0, 5:].any()
    assert phones[int(labels[1, 0]) - 1] == 'T' and not labels[1, 1:].any() and not labels[2].any()
    fold = stress_fold(hp.symbols)
    assert fold.shape == (70,) and fold[0] == 0 and len(set(fold.tolist())) == 1 + 15 + 24
    cls = lambda p: phones.index(p) + 1
    assert fold[cls('AH1')] == fold[cls('AH2')] == fold[cls('AH0')] == cls('AH0') and fold[cls('HH')] == cls('HH')
    assert fold[cls('AA0')] != fold[cls('AE0')]
    toy = Recognizer(O.TOY_SYMBOLS, 4, hidden=8, layers=1)
    assert toy.phones == O.TOY_SYMBOLS[O.TOY_FIRST:] and toy.class_of.tolist() == [0, 0, 0, 0] + list(range(1, 16))


def test_steps_are_the_ceiling_of_frames_over_stride():
    from daft_exprt.recognizer import Recognizer
    n = torch.tensor([0, 1, 2, 3, 4, 5, 999, 1000])
    assert Recognizer(O.TOY_SYMBOLS, 4, hidden=8, layers=1, stride=2).n_steps_of(n).tolist() == [0, 1, 1, 2, 2, 3, 500, 500]
    assert Recognizer(O.TOY_SYMBOLS, 4, hidden=8, layers=1, stride=3).n_steps_of(n).tolist() == [0, 1, 1, 1, 2, 2, 333, 334]
    assert Recognizer(O.TOY_SYMBOLS, 4, hidden=8, layers=1, stride=1).n_steps_of(n).tolist() == n.tolist()
    rec = Recognizer(O.TOY_SYMBOLS, 4, hidden=8, layers=2, stride=2)
    logits, n_steps = rec(torch.randn(2, 4, 7), torch.tensor([7, 4]))
    assert logits.shape == (2, 4, 16) and n_steps.tolist() == [4, 2] and logits.is_contiguous() and logits.dtype == torch.float32


@pytest.mark.parametrize('stride', (1, 2, 3))
def test_forward_batched_equals_alone(stride):
    ''' masked at the sequence end in front of every convolution, and normalised over its own frames: the live steps of a row do
        not depend on the padding, on what lies in it, or on the rows beside it (allclose: a batched matrix product need not round
        like a single one) '''
    from daft_exprt.recognizer import Recognizer
    torch.manual_seed(0)
    rec = Recognizer(O.TOY_SYMBOLS, 6, hidden=16, layers=3, stride=stride).eval()
    n = torch.tensor([13, 8, 1, 7])
    mel = torch.randn(4, 6, 13) * 3.0 - 5.0
    dirty = mel.clone()
    for b in range(4):
        dirty[b, :, int(n[b]):] = float('nan') if b % 2 else 1e4                            # dead frames: never read into a live step
    with torch.no_grad():
        logits, n_steps = rec(dirty, n)
        assert n_steps.tolist() == [-(-int(v) // stride) for v in n]
        for b in range(4):
            alone, steps = rec(mel[b:b + 1, :, :int(n[b])].contiguous(), n[b:b + 1])
            assert int(steps) == int(n_steps[b]) == alone.shape[1]
            assert torch.isfinite(alone).all() and torch.allclose(logits[b, :int(steps)], alone[0], rtol=1e-4, atol=1e-5), b
        x = rec.normalise(dirty, n)
        for b in range(4):
            live = x[b, :int(n[b])]
            assert not x[b, int(n[b]):].any() and torch.allclose(live.mean(0), torch.zeros(6), atol=1e-5)
            if int(n[b]) > 1:
                assert torch.allclose((live * live).mean(0), torch.ones(6), atol=1e-3)


def test_the_loss_wrapper_needs_a_gpu():
    from daft_exprt.recognizer import edit_distance, uctc_greedy
    with pytest.raises(RuntimeError, match='device tensors'):                            # no CPU fallback
        uctc_greedy(torch.zeros(1, 2, 3), torch.tensor([2]))
    with pytest.raises(RuntimeError, match='device tensors'):
        edit_distance(torch.zeros((1, 2), dtype=torch.int32), torch.tensor([2]), torch.zeros((1, 2), dtype=torch.int32), torch.tensor([2]))


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------

def test_limits_and_symbols_through_the_abi():
    from daft_exprt import _hip as H
    from daft_exprt.recognizer import edit_max_len, limits
    lib = H.lib()
    assert lib.dx_abi_version() == 13
    assert limits() == (lib.dx_uctc_max_steps(), lib.dx_uctc_max_labels(), lib.dx_uctc_max_classes()) == (2048, 255, 128)
    assert edit_max_len() == lib.dx_edit_max_len() == 2048
    declared = {name for name, _, _ in H.header_prototypes()}
    assert {'dx_uctc_max_steps', 'dx_uctc_max_labels', 'dx_uctc_max_classes', 'dx_edit_max_len', 'dx_uctc_loss', 'dx_uctc_greedy',
            'dx_edit_distance'} <= declared
    for T, U, V in ((2049, 1, 4), (8, 256, 4), (8, 1, 129)):
        assert lib.dx_uctc_loss(8, 8, 8, 8, 8, 8, 8, 8, 8, 1, T, U, V, None) == -5 and b'at most' in lib.dx_last_error()
    assert lib.dx_uctc_greedy(8, 8, 8, 8, 8, 1, 2049, 4, None) == -5 and lib.dx_uctc_greedy(8, 8, 8, 8, 8, 1, 8, 129, None) == -5
    assert lib.dx_edit_distance(8, 8, 8, 8, 8, 1, 2049, 4, None) == -5 and lib.dx_edit_distance(8, 8, 8, 8, 8, 1, 4, 2049, None) == -5
    assert lib.dx_uctc_loss(None, 8, 8, 8, 8, 8, 8, 8, 8, 1, 8, 1, 4, None) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_edit_distance(None, 8, 8, 8, 8, 1, 4, 4, None) == -1 and lib.dx_edit_distance(8, 8, 8, 8, None, 1, 4, 4, None) == -1
