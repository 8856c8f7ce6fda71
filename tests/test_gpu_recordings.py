"""daft_exprt/recordings.py on the GPU, with the random-init model and the fabricated recordings of
tests/test_gpu_prosody_targets.py: `copy_inference` against `DaftExprt.inference` on the batch sorted by hand, the one front end
behind both `align_batch` functions, and `sounding_crops` on energies handed in.  Everything here is bit for bit: the shared pieces
reorder and select rows, they compute nothing of their own."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_gpu_prosody_targets as TP

DEV = 'cuda:0'


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize('wrapped', [False, True], ids=['the model', 'an object that only has .module'])
def test_copy_inference_equals_inference_on_the_hand_sorted_batch(wrapped):
    from daft_exprt.recordings import copy_inference
    model, hp = TP._model()
    batch = [t.to(DEV) for t in TP._batch(0.)]                           # sorted: 12, 9 and 7 symbols
    assert batch[4].tolist() == [12, 9, 7]
    want_enc, (want_mel, want_n), want_alignments = model.inference(tuple(batch), 'add', hp)
    rows = [2, 0, 1]                                                     # the caller's order: 7, 12 and 9 symbols
    symbols, lengths, energy, pitch, mel, n_rec, speakers = (batch[k][rows] for k in (0, 4, 5, 6, 7, 8, 9))
    symbols = torch.cat([symbols, torch.zeros((3, 2), dtype=torch.int64, device=DEV)], dim=1)        # wider than the longest row
    assert lengths.tolist() == [7, 12, 9]
    try:
        for training in (True, False):
            model.train(training)
            enc, (got_mel, got_n), alignments, order = copy_inference(SimpleNamespace(module=model) if wrapped else model, symbols, lengths,
                                                                      energy, pitch, mel, n_rec, speakers, hp)
            assert model.training == training
            assert order.tolist() == [1, 2, 0] and len(enc) == len(want_enc)
            for got, want in zip(list(enc) + [got_mel, got_n, alignments], list(want_enc) + [want_mel, want_n, want_alignments]):
                assert _same(got, want[rows])
    finally:
        model.eval()


def _recordings(hp, tmp_path):
    ''' the inputs of both `align_batch` functions: the three UTTERANCES, the recording of 400 samples, and one that is not read
        because its sample count says it is longer than the DTW takes '''
    from daft_exprt.evaluate import max_dtw_length
    _, sentences, _ = TP._sentences(tmp_path, True)
    symbols, lengths, wavs, n_samples, speakers = TP._clone_inputs(hp, sentences, TP._waves(True))[:5]
    symbols, lengths, speakers = torch.cat([symbols, symbols[:1]]), torch.cat([lengths, lengths[:1]]), torch.cat([speakers, speakers[:1]])
    wavs = torch.cat([wavs, torch.zeros_like(wavs[:1])])
    return symbols, lengths, wavs, n_samples + [(max_dtw_length() + 1) * hp.hop_length], speakers


def test_both_aligners_stand_on_one_front_end(tmp_path):
    from daft_exprt.align import align_batch
    from daft_exprt.aligner import Aligner
    model, hp = TP._model()
    inputs = _recordings(hp, tmp_path)
    torch.manual_seed(2)
    aligner = Aligner(len(hp.symbols), hp.n_mel_channels, hidden=32, att_dim=16).to(DEV)
    a, b = align_batch(model, *inputs, hp), aligner.align_batch(*inputs, hp)
    sa, sb = a['status'].tolist(), b['status'].tolist()
    print(f'status {sa} / {sb}, begin {a["begin"].tolist()} / {b["begin"].tolist()}, frames {a["frames"].tolist()} / {b["frames"].tolist()}')
    assert sa[:3] == [0, 0, 0] and sa[3:] == sb[3:] == [4, 3]
    assert a['begin'].tolist() == b['begin'].tolist() and a['begin'][0] > 0
    for row in range(5):
        if sa[row] == 0 and sb[row] == 0:
            assert int(a['frames'][row]) == int(b['frames'][row]) > 0
        if sa[row] in (3, 4) or sb[row] in (3, 4):
            assert sa[row] == sb[row]


def test_sounding_crops_on_energies_handed_in(tmp_path):
    from daft_exprt.extract_features import mel_spectrogram_batch
    from daft_exprt.recordings import sounding_crops
    _, hp = TP._model()
    _, _, wavs, n_samples, _ = _recordings(hp, tmp_path)
    for rows in ([0, 1, 2], [0, 1, 2, 3, 4]):                            # every row goes through; two rows are decided before
        sub, n = wavs[rows].contiguous(), [n_samples[b] for b in rows]
        own = sounding_crops(sub, n, hp, -40.0)
        # the energies of the rows as they are (a row that is too short or not there is analysed as one window of what there is)
        seen = [min(max(c, hp.filter_length), sub.shape[1]) for c in n]
        _, energy, n_frames = mel_spectrogram_batch(sub, torch.tensor(seen, dtype=torch.int64, device=DEV), hp, min_samples=min(seen))
        given = sounding_crops(sub, n, hp, -40.0, energy, n_frames)
        (status, kept, begin, cropped, lengths, crop), (*host, cropped_given, _, crop_given) = own, given
        assert status == [0, 0, 0, 4, 3][:len(rows)] and kept == [0, 1, 2] and begin[0] > 0 and cropped.shape == (3, max(lengths))
        assert host == [status, kept, begin] and given[4] == lengths and _same(cropped, cropped_given) and _same(crop, crop_given)
        assert crop.tolist() == [[b * hp.hop_length, n] for b, n in zip(begin, lengths)]
