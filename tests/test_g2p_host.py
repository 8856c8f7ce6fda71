"""The host side of the g2p front end, without a GPU: tests/ctc_oracle.py is pinned against an enumeration of all
alignments and against `torch.nn.functional.ctc_loss` in float64 on the shapes of tests/test_gpu_g2p.py; daft_exprt/text.py against
what the imported reference recorded (tests/golden/text_frontend.json, tools/gen_golden_text.py) and against a table of number
expansions written from the rules of the reference's `normalize_numbers.py`."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ctc_oracle as O
from tests.util import make_hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'text_frontend.json')


# ---- the oracle --------------------------------------------------------------------------------------------------------------------------

def test_oracle_loss_equals_the_sum_over_all_alignments():
    ''' every label sequence with T <= 5, V <= 3, U <= 3, repeats included: the recurrence against V ** T enumerated paths '''
    rng = np.random.RandomState(0)
    checked = infeasible = 0
    for T, V, U in itertools.product(range(1, 6), (2, 3), range(0, 4)):
        x = rng.standard_normal((1, T, V))
        for labels in itertools.product(range(1, V), repeat=U):
            lab = np.array([list(labels) + [0] * (3 - U)], dtype=np.int64)
            loss, status, grad = O.ctc_loss(x, [T], lab, [U])
            want = O.enumerate_loss(x[0], labels)
            assert status[0] == (0 if np.isfinite(want) else 1), (T, V, labels)
            if status[0] == 0:
                assert abs(loss[0] - want) < 1e-12 * max(1.0, abs(want)), (T, V, labels, loss[0], want)
                assert np.abs(grad[0].sum(axis=1)).max() < 1e-12           # softmax minus posteriors: every step sums to 0
                checked += 1
            else:
                assert np.isnan(loss[0]) and not grad.any()
                infeasible += 1
    assert checked + infeasible == 5 * (4 + 15) and checked > 50 and infeasible > 30


@pytest.mark.parametrize('V', O.CLASSES)
def test_oracle_equals_torch_ctc_loss_on_the_gpu_shapes(V):
    c = O.gpu_case(V)
    loss, status, grad = O.ctc_loss(c['logits'], c['n_steps'], c['labels'], c['n_labels'], c['w'])
    assert status.tolist() == c['status'].tolist()
    ok = [b for b in range(c['B']) if status[b] == 0]
    x = torch.tensor(c['logits'][ok], dtype=torch.float64, requires_grad=True)
    per = F.ctc_loss(F.log_softmax(x, dim=2).transpose(0, 1), torch.tensor(c['labels'][ok]), torch.tensor(c['n_steps'][ok]),
                     torch.tensor(c['n_labels'][ok]), blank=0, reduction='none')
    (per * torch.tensor(c['w'][ok], dtype=torch.float64)).sum().backward()
    assert np.abs(loss[ok] - per.detach().numpy()).max() < 1e-9 * np.abs(loss[ok]).max()
    want = x.grad.numpy()
    for i, b in enumerate(ok):
        nT = int(c['n_steps'][b])
        assert np.abs(grad[b, :nT] - want[i, :nT]).max() < 1e-9, (V, b)
        assert not grad[b, nT:].any()
    for b in range(c['B']):
        if status[b] != 0:
            assert np.isnan(loss[b]) and not grad[b].any()


def test_status_rules():
    assert O.status_of(0, [1, 2], 5) == 2 and O.status_of(0, [], 5) == 2             # no step: decided first
    assert O.status_of(1, [], 5) == 0                                                 # no label: the all-blank path
    assert O.status_of(3, [1, 1], 5) == 0 and O.status_of(2, [1, 1], 5) == 1          # equal neighbours need a blank between
    assert O.status_of(2, [1, 2], 5) == 0 and O.status_of(1, [1, 2], 5) == 1
    assert O.status_of(5, [1, 1, 1], 5) == 0 and O.status_of(4, [1, 1, 1], 5) == 1
    assert O.status_of(9, [1, 5], 5) == 3 and O.status_of(9, [0], 5) == 3            # a label outside [1, V - 1]
    x = np.zeros((3, 4, 3))
    loss, status, grad = O.ctc_loss(x, [4, 0, 1], np.array([[1, 2], [1, 0], [2, 2]]), [2, 1, 2])
    assert status.tolist() == [0, 2, 1] and np.isfinite(loss[0]) and np.isnan(loss[1:]).all() and not grad[1:].any()
    loss, _, grad = O.ctc_loss(x[:1], [4], np.zeros((1, 1), dtype=np.int64), [0])     # all blank: 4 log 3
    assert abs(loss[0] - 4 * np.log(3)) < 1e-12 and np.abs(grad[0, :, 0] - (1 / 3 - 1)).max() < 1e-12


def test_greedy_oracle():
    x = np.full((2, 9, 4), -4.0)
    for t, c in enumerate([1, 1, 0, 1, 2, 2, 0, 0, 3]):
        x[0, t, c] = 0.0
    x[1, :, :] = 0.0                                                                  # all tied: the lowest class, the blank
    x[1, 3, 2] = x[1, 3, 3] = 1.0                                                     # a tie between 2 and 3: 2
    ids, n_out, score = O.greedy(x, [9, 6])
    assert ids[0].tolist() == [1, 1, 2, 3, 0, 0, 0, 0, 0] and n_out.tolist() == [4, 1] and ids[1, 0] == 2 and not ids[1, 1:].any()
    assert abs(score[0] + 9 * np.log(1 + 3 * np.exp(-4.0))) < 1e-12
    assert O.greedy(x, [0, 0])[1].tolist() == [0, 0]


def test_toy_lexicon_rules_and_feasibility():
    assert O.toy_pronounce('shot') == ['SH', 'AA1', 'T'] and O.toy_pronounce('bitte') == ['B', 'IH1', 'T', 'EH1']
    assert O.toy_pronounce('bite') == ['B', 'AY1', 'T'] and O.toy_pronounce('axe') == ['EY1', 'K', 'S']
    assert O.toy_pronounce('kit') == ['S', 'IH1', 'T'] and O.toy_pronounce('kot') == ['K', 'AA1', 'T']
    assert O.toy_pronounce('khat') == ['CH', 'AE1', 'T'] and O.toy_pronounce('aa') == ['AE1', 'AE1']
    lexicon = O.toy_lexicon()
    assert len(lexicon) == 2000 == len({w for w, _ in lexicon}) and lexicon == O.toy_lexicon()
    for word, phones in lexicon:
        assert 2 <= len(word) <= 10 and phones and set(word) <= set(O.TOY_LETTERS)
        assert len(phones) + O.repeats_of(phones) <= 3 * len(word)                    # a CTC path with 3 slots per letter
    assert set(p for _, ps in lexicon for p in ps) == set(O.TOY_PHONES)


def test_limits_are_refused_before_any_launch():
    from daft_exprt import _hip as H
    lib = H.lib()
    assert (lib.dx_ctc_max_steps(), lib.dx_ctc_max_labels(), lib.dx_ctc_max_classes()) == (256, 127, 128)
    for T, U, V in ((257, 1, 4), (8, 128, 4), (8, 1, 129)):
        assert lib.dx_ctc_loss(8, 8, 8, 8, 8, 8, 8, 8, 8, 1, T, U, V, None) == -5 and b'at most' in lib.dx_last_error()
    assert lib.dx_ctc_greedy(8, 8, 8, 8, 8, 1, 257, 4, None) == -5 and lib.dx_ctc_greedy(8, 8, 8, 8, 8, 1, 8, 129, None) == -5
    assert lib.dx_ctc_loss(None, 8, 8, 8, 8, 8, 8, 8, 8, 1, 8, 1, 4, None) == -1 and b'null' in lib.dx_last_error()
    with pytest.raises(RuntimeError, match='device tensors'):                          # no CPU fallback
        from daft_exprt.g2p import ctc_greedy
        ctc_greedy(torch.zeros(1, 2, 3), torch.tensor([2]))


def test_error_rates():
    from daft_exprt.g2p import error_rates
    per, wer = error_rates([['A', 'B'], None, ['C']], [[['A', 'B']], [['X', 'Y']], [['C', 'D'], ['C']]])
    assert per == 2 / 5 and wer == 1 / 3


def test_batches_are_one_permutation_per_epoch_sorted_by_length():
    from daft_exprt.g2p import length_sorted_batches
    lengths = [3, 9, 4, 4, 2, 7, 5, 8, 6, 2]
    draw = lambda seed: length_sorted_batches(lengths, 4, torch.Generator().manual_seed(seed))
    batches, again = draw(1), draw(1)
    for _ in range(3):                                                                # three epochs of 4 + 4 + 2
        epoch = [next(batches) for _ in range(3)]
        assert [len(idx) for idx, _ in epoch] == [4, 4, 2]
        assert sorted(i for idx, _ in epoch for i in idx.tolist()) == list(range(10))
        for idx, longest in epoch:
            own = [lengths[i] for i in idx.tolist()]
            assert own == sorted(own) and longest == own[-1] and idx.dtype == torch.int64
            assert next(again)[0].tolist() == idx.tolist()                            # seeded
    assert [next(draw(1))[0].tolist() for _ in range(2)] != [next(draw(2))[0].tolist() for _ in range(2)]


def test_train_g2p_names_the_word_of_an_unknown_phone():
    from daft_exprt.g2p import train_g2p
    with pytest.raises(ValueError, match='unknown phone "QQ".*"odd"'):
        train_g2p({'fine': [['F', 'AY1', 'N']], 'odd': [['AA1', 'QQ']]}, make_hparams(), steps=1)


# ---- the dictionary ----------------------------------------------------------------------------------------------------------------------

def test_load_dictionary(tmp_path):
    from daft_exprt.text import load_dictionary
    path = tmp_path / 'english.dict'
    path.write_text(';;; a comment\nHELLO HH AH0 L OW1\nhello(2)  HH EH0 L OW1\n\nworld W ER1 L D\nHello HH AH0 L OW1\n'
                    "don't D OW1 N T\n", encoding='utf-8')
    d = load_dictionary(str(path), make_hparams().symbols)
    assert d == {'hello': [['HH', 'AH0', 'L', 'OW1'], ['HH', 'EH0', 'L', 'OW1']], 'world': [['W', 'ER1', 'L', 'D']],
                 "don't": [['D', 'OW1', 'N', 'T']]}
    bad = tmp_path / 'bad.dict'
    bad.write_text('fine F AY1 N\nodd AA1 QQ D\n', encoding='utf-8')
    with pytest.raises(ValueError, match=r'line 2.*QQ'):
        load_dictionary(str(bad))
    bad.write_text('empty\n', encoding='utf-8')
    with pytest.raises(ValueError, match='line 1'):
        load_dictionary(str(bad))


# ---- the cleaner and the sentence splitter against the reference's recorded outputs ------------------------------------------------------

def _golden():
    with open(GOLDEN, 'r', encoding='utf-8') as f:
        return json.load(f)


def test_text_cleaner_against_the_reference():
    from daft_exprt.text import text_cleaner
    cases = _golden()['text_cleaner']
    assert len(cases) >= 10
    for case in cases:
        assert text_cleaner(case['text'], 'english') == case['cleaned'], case['text']
    assert text_cleaner('Mr. X', 'french') == 'Mr. X'


def test_phonemize_sentence_against_the_reference():
    from daft_exprt.generate import phonemize_sentence                               # the reference's import path
    from daft_exprt.symbols import eos
    fx = _golden()
    hp = make_hparams()
    dictionary = {word: [phones] for word, phones in fx['dictionary'].items()}
    assert fx['phonemize_sentence'][0]['sentence'] == "that's, an 'example! ' of a sentence. '"
    for case in fx['phonemize_sentence']:
        got = phonemize_sentence(case['sentence'], hp, dictionary)
        assert got == case['phonemized'], case['sentence']
        assert got[-1] == eos and isinstance(got[0], list)


def test_first_pronunciation_unless_an_rng_is_given():
    import random
    from daft_exprt.text import phonemize_sentence
    hp = make_hparams()
    d = {'read': [['R', 'IY1', 'D'], ['R', 'EH1', 'D']]}
    assert phonemize_sentence('read.', hp, d) == [['R', 'IY1', 'D'], '.', '~']
    seen = {tuple(phonemize_sentence('read.', hp, d, rng=random.Random(s))[0]) for s in range(20)}
    assert seen == {('R', 'IY1', 'D'), ('R', 'EH1', 'D')}
    assert phonemize_sentence('read read', hp, d) == [['R', 'IY1', 'D'], ' ', ['R', 'IY1', 'D'], '~']    # no closing mark: none invented


NUMBERS = (('1,000', 'one thousand'), ('3.5', 'three point five'), ('$3.50', 'three dollars, fifty cents'), ('£2', 'two pounds'),
           ('2nd', 'second'), ('1999', 'nineteen ninety-nine'), ('2005', 'two thousand five'), ('1000000', 'one million'),
           ('21st', 'twenty-first'), ('101st', 'one hundred and first'), ('1905', 'nineteen oh five'), ('1800', 'eighteen hundred'),
           ('2000', 'two thousand'), ('$1', 'one dollar'), ('$0.01', 'one cent'), ('42', 'forty-two'), ('0', 'zero'),
           ('999999999999', 'nine hundred ninety-nine billion, nine hundred ninety-nine million, nine hundred ninety-nine thousand, '
                            'nine hundred ninety-nine'),
           ('3000', 'three thousand'), ('1,234,567', 'one million, two hundred thirty-four thousand, five hundred sixty-seven'))


def test_number_expansion_table():
    ''' written from the rules of normalize_numbers.py and the wording of the inflect package (commas between the groups of three,
        hyphenated tens-units, no "and" in cardinals, "and" in ordinals); the cleaner then turns the hyphens into spaces '''
    from daft_exprt.text import normalize_numbers, text_cleaner
    for text, want in NUMBERS:
        assert normalize_numbers(text) == want, text
        assert text_cleaner(f'It is {text} now.') == f'it is {want.replace("-", " ")} now.', text


# ---- files -------------------------------------------------------------------------------------------------------------------------------

class _FakeG2P:
    ''' stands in for `g2p.G2P.phonemize` (the model itself needs a GPU): spells a word letter by letter, knows no q '''
    calls = 0

    def phonemize(self, words, batch_size=None):
        self.calls += 1
        table = {'z': 'Z', 'o': 'OW1', 'g': 'G'}
        return [None if 'q' in w else [table.get(c, 'AH0') for c in w] for w in words]


def test_prepare_sentences_round_trip(tmp_path):
    from daft_exprt.generate import prepare_sentences_for_inference, read_phonemised_sentences
    fx = _golden()
    hp = make_hparams()
    dictionary = {word: [phones] for word, phones in fx['dictionary'].items()}
    text = tmp_path / 'lines.txt'
    text.write_text('Hello there, world!\n\nutt_7|Wait... what? zog the zog.\nyes\n', encoding='utf-8')
    out = tmp_path / 'out'
    out.mkdir()
    (out / 'keep.me').write_text('x', encoding='utf-8')
    g2p, report = _FakeG2P(), {}
    sentences, names = prepare_sentences_for_inference(str(text), str(out), hp, g2p=g2p, dictionary=dictionary, report=report)
    assert names == ['lines.txt_line0', 'utt_7', 'lines.txt_line3'] and (out / 'keep.me').is_file()    # the directory is not deleted
    assert g2p.calls == 1 and report == {'oov': {'zog': ['Z', 'OW1', 'G']}, 'dictionary_words': 7}       # one batch for all sentences
    back, back_names = read_phonemised_sentences(str(out / 'sentences_to_generate.txt'), hp.symbols)
    assert back == sentences and back_names == names
    assert sentences[1] == [fx['dictionary']['wait'], '.', fx['dictionary']['what'], '?', ['Z', 'OW1', 'G'], ' ', fx['dictionary']['the'],
                            ' ', ['Z', 'OW1', 'G'], '.', '~']


def test_oov_without_a_g2p_raises_and_names_the_words(tmp_path):
    from daft_exprt.text import phonemize_sentence, prepare_sentences_for_inference
    hp = make_hparams()
    dictionary = {'the': [['DH', 'AH0']]}
    with pytest.raises(ValueError, match='no g2p model.*quux, zog'):
        phonemize_sentence('The zog, the quux.', hp, dictionary)
    with pytest.raises(ValueError, match='gives no phones.*: quux$'):
        phonemize_sentence('The zog, the quux.', hp, dictionary, g2p=_FakeG2P())
    text = tmp_path / 'lines.txt'
    text.write_text('the zog\n', encoding='utf-8')
    with pytest.raises(ValueError, match='zog'):
        prepare_sentences_for_inference(str(text), str(tmp_path / 'out'), hp, dictionary=dictionary)
    assert not (tmp_path / 'out' / 'sentences_to_generate.txt').exists()
    with pytest.raises(ValueError, match='no word'):
        phonemize_sentence(' ... ', hp, dictionary)


def test_synthesize_help_still_lists_the_old_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'synthesize.py'), '--help'], capture_output=True, text=True,
                         check=True).stdout
    for flag in ('-out OUTPUT_DIR', '-chk CHECKPOINT', '-tf TEXT_FILE', '-sb', '[-bs BATCH_SIZE]', '[-rtf]', '[-ctrl]', '[-voc VOCODER]',
                 '[-vcfg VOCODER_CONFIG]', '[-dict DICTIONARY]', '[-g2p G2P]'):
        assert flag in out, flag
