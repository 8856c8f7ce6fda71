"""Host side of daft_exprt/recordings.py: the pieces `align`, `aligner`, `clone`, `evaluate` and `generate` share.  A span in frames
as a crop in samples and the statuses decided before any launch, reference triples padded into batch tensors, the three forms of
`phonemised_files`, and the sort `copy_inference` applies for `DaftExprt.inference` and undoes again.  Nothing here needs the
HIP library or a GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from daft_exprt import recordings as R

HOP, N_FFT = 256, 1024
HALF = N_FFT // 2
HP = SimpleNamespace(hop_length=HOP, filter_length=N_FFT, centered=True, n_mel_channels=80)


#                        name                                        span      n_samples        want
@pytest.mark.parametrize('name, span, n, want', [
    ('exactly half a window: no crop',                              (0, 2),   5000,            4),
    ('exactly half a window after the clamp: no crop',              (1, 10),  HOP + HALF,      4),
    ('half a window and one sample',                                (1, 10),  HOP + HALF + 1,  (1, HOP, HALF + 1)),
    ('the end is clamped to the recording',                         (2, 10),  2000,            (2, 2 * HOP, 2000 - 2 * HOP)),
    ('the end at a hop multiple inside the recording',              (3, 9),   5000,            (3, 3 * HOP, 6 * HOP)),
    ('an empty span',                                               (0, 0),   5000,            4),
    ('a one-frame span',                                            (7, 8),   5000,            4),
])
def test_span_crops(name, span, n, want):
    assert R.span_crops([span], [n], HOP, N_FFT) == [want], name
    # a row's answer does not depend on its neighbours
    assert R.span_crops([(0, 4), span, (0, 0)], [5000, n, 5000], HOP, N_FFT) == [(0, 0, 4 * HOP), want, 4], name


def test_statuses_decided_before_any_launch(monkeypatch):
    monkeypatch.setattr(R, 'max_dtw_length', lambda: 100)                # (the library's limit: not needed here)
    over = 100 * HOP                                                     # 1 + n // hop frames with `centered`: 101
    assert R.early_statuses([HALF, HALF + 1, over - 1, over, 0], HP) == [4, 0, 0, 3, 4]
    # `sounding_crops` consults no span -- launches nothing -- where every row is decided here: host tensors pass
    crops = R.sounding_crops(torch.zeros((3, 8)), [HALF, over, 1], HP, -40.0)
    assert crops == ([4, 3, 4], [], [], None, None, None)
    with pytest.raises(ValueError, match='centered'):
        R.sounding_crops(torch.zeros((1, 8)), [HALF], SimpleNamespace(hop_length=HOP, filter_length=N_FFT, centered=False), -40.0)


def test_early_statuses_go_into_an_empty_alignment():
    out = R.empty_alignment(4, 5, 'cpu')
    assert tuple(out) == R.ALIGN_KEYS
    assert [tuple(out[k].shape) for k in R.ALIGN_KEYS] == [(4,), (4, 5), (4, 5), (4,), (4,), (4,), (4,), (4,)]
    assert torch.isnan(out['path_cost']).all() and not any(out[k].any() for k in R.ALIGN_KEYS if k != 'path_cost')
    out['status'][2] = 1                                                 # (a status written on the device stays)
    R.write_early_statuses(out, [0, 4, 0, 3])
    assert out['status'].tolist() == [0, 4, 1, 3] and out['status'].dtype == torch.int32
    R.write_early_statuses(out, [0, 0, 0, 0])
    assert out['status'].tolist() == [0, 4, 1, 3]


def test_pad_references():
    rng = np.random.RandomState(0)
    frames = [5, 9, 1]
    triples = [(rng.rand(t).astype(np.float32) + 1, rng.rand(t).astype(np.float32) + 1, rng.rand(3, t).astype(np.float32) + 1) for t in frames]
    energy, pitch, mel, n_rec = R.pad_references(triples, "cpu")
    assert energy.shape == pitch.shape == (3, 9) and mel.shape == (3, 3, 9) and energy.dtype == pitch.dtype == mel.dtype == torch.float32
    assert n_rec.tolist() == frames and n_rec.dtype == torch.int64
    for b, (t, (e, p, m)) in enumerate(zip(frames, triples)):
        assert energy[b, :t].numpy().tobytes() == e.tobytes() and pitch[b, :t].numpy().tobytes() == p.tobytes()
        assert mel[b, :, :t].numpy().tobytes() == m.tobytes()
        assert not energy[b, t:].any() and not pitch[b, t:].any() and not mel[b, :, t:].any()


def test_phonemised_files_in_their_three_forms(tmp_path):
    speakers = ['a', 'b']
    assert R.phonemised_by_speaker('all.txt', speakers) == {'a': 'all.txt', 'b': 'all.txt'}
    assert R.phonemised_by_speaker(tmp_path / 'all.txt', speakers) == {'a': tmp_path / 'all.txt', 'b': tmp_path / 'all.txt'}
    assert R.phonemised_by_speaker(['a.txt', 'b.txt'], speakers) == {'a': 'a.txt', 'b': 'b.txt'}
    given = {'a': 'x.txt', 'b': 'y.txt'}
    assert R.phonemised_by_speaker(given, speakers) == given
    with pytest.raises(AssertionError, match='3 phonemised files for 2 speakers'):
        R.phonemised_by_speaker(['a.txt', 'b.txt', 'c.txt'], speakers)


class _Core(object):
    ''' what `copy_inference` touches of a `DaftExprt`; `inference` records its inputs and returns tensors made of them '''
    def __init__(self):
        self.training, self.seen = True, None

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode

    def inference(self, inputs, pitch_transform, hparams, **kw):
        assert not self.training and not torch.is_grad_enabled()
        self.seen = (inputs, pitch_transform, kw)
        symbols, lens, speaker_ids = inputs[0], inputs[4], inputs[9]
        rows = speaker_ids.float()
        enc = (rows[:, None] + symbols.float(), symbols * 2, rows[:, None].expand(symbols.shape), symbols.float(), lens)
        return enc, (rows[:, None, None].expand(-1, 2, 6), inputs[8] + 1), rows[:, None, None].expand(-1, symbols.shape[1], 6)


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('lengths, want', [([7, 11, 8], [1, 2, 0]), ([7, 9, 7, 9], [1, 3, 0, 2]), ([3, 5], [1, 0]), ([4], None),
                                           ([9, 9, 7, 7, 3], None), ([12, 9, 7], None)])
def test_copy_inference_sorts_for_the_model_and_answers_in_the_callers_order(lengths, want, training):
    ''' want: the stable sort, longest first -- None where it leaves the batch in place, ties included '''
    B, L, T = len(lengths), max(lengths) + 2, 5                          # (symbols two columns wider than the longest row)
    symbols = torch.zeros((B, L), dtype=torch.int64)
    for b, n in enumerate(lengths):
        symbols[b, :n] = torch.arange(1, n + 1) + 20 * b
    refs = torch.arange(B * T, dtype=torch.float32).reshape(B, T)
    mel, n_rec, speakers = refs[:, None, :].repeat(1, 2, 1), torch.arange(B) + 3, torch.arange(B)
    core = _Core()
    core.training = training
    enc, (mel_gen, n_gen), alignments, order = R.copy_inference(SimpleNamespace(module=core), symbols, torch.tensor(lengths), refs, refs + 100,
                                                                mel, n_rec, speakers, None)
    assert core.training == training and (order if want is None else order.tolist()) == want
    inputs, transform, kw = core.seen
    assert transform == 'add' and kw == {} and len(inputs) == 10
    assert inputs[4].tolist() == sorted(lengths, reverse=True) and inputs[0].shape == (B, max(lengths))
    assert inputs[1].eq(1).all() and inputs[2].eq(1).all() and inputs[3].eq(0).all() and all(t.is_contiguous() for t in inputs)
    seen = inputs[9].tolist()                                            # the caller's row behind every row of the sorted batch
    assert seen == (list(range(B)) if want is None else want)            # (every row once: the sort is a bijection)
    for k, b in enumerate(seen):
        assert inputs[0][k].tolist() == symbols[b, :max(lengths)].tolist() and inputs[5][k].tolist() == refs[b].tolist()
        assert inputs[6][k].tolist() == (refs[b] + 100).tolist() and torch.equal(inputs[7][k], mel[b]) and inputs[8][k] == n_rec[b]
    # and undone: every output row is the one of the caller's row
    rows = [float(b) for b in range(B)]
    assert enc[4].tolist() == lengths and n_gen.tolist() == (n_rec + 1).tolist()
    assert enc[1].tolist() == (2 * symbols[:, :max(lengths)]).tolist() and enc[2][:, 0].tolist() == rows
    assert mel_gen[:, 0, 0].tolist() == rows and alignments[:, 0, 0].tolist() == rows
