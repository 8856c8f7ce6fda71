"""The validation report's kernels (`csrc/validation.hip`) against `tests/validation_oracle.py`, and the report end to end.

Histogram counts, extremes and flags, and the alignment's frame and hit counts are integers or exact selections: compared exactly.
`mass` is a mean of at most out_length fp32 values in [0, 1]: summed in any order and divided once it lies within
out_length * 2^-23 of the float64 oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util import make_hparams
from tests.validation_oracle import BINS, alignment_oracle, film_hist_oracle, target_alignment_oracle

DEV = 'cuda:0'


def _planted_on_edges():
    ''' gammas on the exactly representable edges 0, 0.125 .. 6.25 with both extremes repeated; betas on the fp32 roundings of the
        edges between two arbitrary fp32 extremes (values that sit a rounding error to either side of their edge), extremes repeated '''
    gam = np.concatenate([np.arange(BINS + 1) * 0.125, [0., 0., 6.25, 6.25]]).astype(np.float32)
    lo, hi = np.float32(-1.3), np.float32(2.7)
    bet = np.concatenate([np.linspace(np.float64(lo), np.float64(hi), BINS + 1).astype(np.float32), [lo, lo, hi, hi]]).astype(np.float32)
    assert bet.min() == lo and bet.max() == hi
    return np.stack([gam, bet], axis=1)[:, None, :]          # (55, 1, 2)


def _random(shape, seed):
    return np.random.default_rng(seed).normal(size=shape).astype(np.float32)


def _constant_group():
    film = _random((4, 2, 6), 5)
    film[:, 0, :3] = np.float32(1.5)
    return film


def _non_finite_groups():
    film = _random((6, 2, 8), 6)
    film[2, 0, 5] = np.inf            # block 0 betas
    film[4, 1, 1] = np.nan            # block 1 gammas
    return film


HIST_CASES = {'one value per group': lambda: _random((1, 1, 2), 1),
              'small': lambda: _random((3, 2, 6), 2),
              'a wave and one': lambda: _random((13, 4, 10), 3),
              'several workgroups': lambda: _random((70, 4, 256), 4),
              'planted on edges': _planted_on_edges,
              'constant group': _constant_group,
              'inf and nan': _non_finite_groups}


@pytest.mark.parametrize('case', list(HIST_CASES))
def test_film_histograms_equal_numpy(case):
    from daft_exprt.validation_report import film_histograms
    film = HIST_CASES[case]()
    counts, edges, minmax, finite = film_hist_oracle(film)
    got = film_histograms(torch.from_numpy(film).to(DEV))
    print(case, 'finite', got['finite'].tolist(), 'count mismatches', int((got['counts'] != counts).sum()))
    assert got['counts'].dtype == np.int64 and got['edges'].dtype == np.float64
    assert np.array_equal(got['finite'], finite)
    assert np.array_equal(got['minmax'], minmax)
    assert np.array_equal(got['edges'], edges)
    assert np.array_equal(got['counts'], counts)
    n = film.shape[0] * film.shape[2] // 2
    assert np.array_equal(got['counts'].sum(-1), np.where(finite, n, 0))
    if case == 'inf and nan':
        assert finite.tolist() == [[True, False], [False, True]]
    if case == 'constant group':
        assert got['counts'][0, 0, BINS // 2] == 12 and got['edges'][0, 0, 0] == 1.0 and got['edges'][0, 0, -1] == 2.0


def _softmax_weights(durations, in_lengths, out_lengths, L, T, seed, tie=None):
    ''' random softmax columns in float64 that lean towards the owner, cast to fp32; no two fp32 values of a column's live rows tie
        for the maximum (the next seed is tried otherwise), then `tie` = (b, t, l0, l1) plants one '''
    B = len(in_lengths)
    while True:
        rng = np.random.default_rng(seed)
        logits = rng.normal(size=(B, L, T))
        for b in range(B):
            logits[b, :, :out_lengths[b]] += 2. * target_alignment_oracle(durations[b], in_lengths[b], out_lengths[b])
        e = np.exp(logits - logits.max(axis=1, keepdims=True))
        w = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
        clean = True
        for b in range(B):
            live = np.sort(w[b, :in_lengths[b], :], axis=0)
            clean &= in_lengths[b] < 2 or bool((live[-1] > live[-2]).all())
        if clean:
            break
        seed += 1
    if tie is not None:
        b, t, l0, l1 = tie
        w[b, l0, t] = w[b, l1, t] = np.float32(min(1., 1.5 * float(w[b, :in_lengths[b], t].max())))
    return w


def _check_alignment(w, durations, in_lengths, out_lengths):
    from daft_exprt.validation_report import alignment_scores
    dev = lambda a, dt: torch.from_numpy(np.asarray(a)).to(dt).to(DEV)
    frames, hits, mass = alignment_scores(dev(w, torch.float32), dev(durations, torch.int64), dev(in_lengths, torch.int64),
                                          dev(out_lengths, torch.int64))
    assert frames.dtype == torch.int64 and hits.dtype == torch.int64 and mass.dtype == torch.float32
    frames, hits, mass = frames.cpu().numpy(), hits.cpu().numpy(), mass.cpu().numpy()
    o_frames, o_hits, o_mass = alignment_oracle(w, durations, in_lengths, out_lengths)
    print('frames', frames.tolist(), 'hits', hits.tolist(), 'oracle hits', o_hits.tolist(),
          'mass error', np.abs(mass.astype(np.float64) - o_mass).tolist(), 'bound', (np.asarray(out_lengths) * 2. ** -23).tolist())
    assert np.array_equal(frames, o_frames) and np.array_equal(hits, o_hits)
    assert (np.abs(mass.astype(np.float64) - o_mass) <= np.asarray(out_lengths) * 2. ** -23).all()
    return frames, hits, mass


def test_alignment_scores_small_batch_with_every_edge():
    B, L, T = 3, 7, 37
    in_lengths, out_lengths = [7, 5, 1], [37, 20, 1]
    durations = np.array([[5, 0, 6, 0, 7, 4, 8],        # zero-duration symbols; 30 frames of 37
                          [6, 5, 0, 7, 9, 3, 2],        # 27 frames cut at 20; the last two symbols are past the input length
                          [0, 0, 0, 0, 0, 0, 0]])       # owns nothing
    # frame 12 of utterance 0 belongs to symbol 4 (frames 11 .. 17); symbols 2 and 4 share its maximum, so the argmax is 2: a miss
    w = _softmax_weights(durations, in_lengths, out_lengths, L, T, seed=11, tie=(0, 12, 2, 4))
    assert np.argmax(w[0, :, 12]) == 2 and w[0, 2, 12] == w[0, 4, 12]
    frames, hits, mass = _check_alignment(w, durations, in_lengths, out_lengths)
    assert frames.tolist() == [30, 20, 0] and mass[2] == 0. and hits[2] == 0
    assert 0 < hits[0] < 30       # the case tells a right argmax from a wrong one


def test_alignment_scores_across_waves():
    B, L, T = 2, 130, 300
    rng = np.random.default_rng(21)
    in_lengths, out_lengths = [130, 97], [300, 211]
    durations = rng.integers(0, 5, size=(B, L))
    w = _softmax_weights(durations, in_lengths, out_lengths, L, T, seed=22)
    frames, hits, _ = _check_alignment(w, durations, in_lengths, out_lengths)
    assert frames[0] == min(int(durations[0].sum()), 300) and frames[1] == min(int(durations[1, :97].sum()), 211)
    assert (hits > 0).all() and (hits < frames).all()


def test_alignment_scores_carry_the_prefix_into_a_second_chunk():
    ''' the kernel scans 256 symbols per chunk: symbols 256 .. 259 get their first frame from the carry of the chunk before.
        Durations of 0 .. 2 sum to about L = 260, below T = 300, so it is utterance 0's own out_length that its sum passes:
        the cut falls inside symbol 258, in the second chunk.  Utterance 1 ends on the second chunk's first symbol. '''
    B, L, T = 2, 260, 300
    durations = np.random.default_rng(31).integers(0, 3, size=(B, L))
    durations[0, 256:] = [1, 0, 2, 2]
    durations[1, 256] = 2
    in_lengths = [260, 257]
    out_lengths = [int(durations[0, :256].sum()) + 2, 300]
    assert durations[0, :256].sum() < out_lengths[0] < durations[0].sum() and durations[1, :257].sum() <= 300
    w = _softmax_weights(durations, in_lengths, out_lengths, L, T, seed=32)
    frames, hits, _ = _check_alignment(w, durations, in_lengths, out_lengths)
    assert frames.tolist() == [out_lengths[0], int(durations[1, :257].sum())]
    assert (hits > 0).all() and (hits < frames).all()


def test_validate_with_a_report_matches_the_oracle(tmp_path):
    ''' 2-block, 2-speaker model, two batches of 3 utterances with T <= 64: the written report equals the oracle applied to the same
        model outputs fetched to the host, and the losses are those of `validate` without a report, bit for bit '''
    from daft_exprt.data_loader import synthetic_batch
    from daft_exprt.loss import DaftExprtLoss
    from daft_exprt.model import DaftExprt
    from daft_exprt.train import validate
    from daft_exprt.validation_report import MODULES, ValidationReport
    hp = make_hparams(speakers=['spkA', 'spkB'], batch_size=3)
    for cfg in (hp.prosody_encoder, hp.phoneme_encoder, hp.frame_decoder):
        cfg['nb_blocks'] = 2
    torch.manual_seed(7)
    model = DaftExprt(hp).to(DEV)
    criterion = DaftExprtLoss(0, hp)
    loader = [synthetic_batch(hp, 3, seed=41 + i, t_max=64, force_first_full=False, l_range=(8, 20)) for i in range(2)]
    plain = validate(0, model, criterion, loader, hp)
    report = ValidationReport(hp, 5, len(loader))
    with_report = validate(0, model, criterion, loader, hp, report=report)
    assert plain[0] == with_report[0] and plain[1] == with_report[1]
    assert model.training
    scalars = report.write(str(tmp_path / 'validation'))
    got = np.load(tmp_path / 'validation' / 'iter_0000005.npz')

    films, frames, hits, mass, bound, kept = {m: [] for m in MODULES}, [], [], [], [], []
    model.eval()
    with torch.no_grad():
        for batch in loader:
            inputs, targets, _ = model.parse_batch(0, batch)
            outputs = model(inputs)
            for m, film in zip(MODULES, outputs[1][1:4]):
                films[m].append(film.float().cpu().numpy())
            w, dint, n_in, n_out = outputs[4].float().cpu().numpy(), inputs[2].cpu().numpy(), inputs[5].cpu().numpy(), inputs[9].cpu().numpy()
            f, h, ms = alignment_oracle(w, dint, n_in, n_out)
            frames.append(f), hits.append(h), mass.append(ms), bound.append(n_out * 2. ** -23)
            kept.append((inputs, targets, outputs))
    model.train()
    for m in MODULES:
        counts, edges, _, finite = film_hist_oracle(np.concatenate(films[m]))
        assert counts.shape[0] == (1 if m == 'prosody_predictor' else 2) and finite.all()
        assert np.array_equal(got[f'film_{m}_counts'], counts) and np.array_equal(got[f'film_{m}_edges'], edges)
        assert np.array_equal(got[f'film_{m}_finite'], finite)
        halves = np.concatenate(films[m]).astype(np.float64)
        halves = halves.reshape(halves.shape[0], halves.shape[1], 2, -1)
        assert np.allclose(got[f'film_{m}_mean'], halves.mean(axis=(0, 3)), rtol=1e-12, atol=1e-12)
        assert np.allclose(got[f'film_{m}_std'], halves.std(axis=(0, 3)), rtol=1e-9, atol=1e-12)
    frames, hits, mass, bound = (np.concatenate(x) for x in (frames, hits, mass, bound))
    err = np.abs(got['alignment_mass'].astype(np.float64) - mass)
    print('frames', frames.tolist(), 'hits', hits.tolist(), 'mass error', err.tolist(), 'bound', bound.tolist())
    assert np.array_equal(got['alignment_frames'], frames) and np.array_equal(got['alignment_hits'], hits)
    assert (err <= bound).all() and (frames > 0).all()
    assert scalars['DaftExprt.validation/alignment_hit_rate'] == float(hits.sum()) / float(frames.sum())
    assert abs(scalars['DaftExprt.validation/alignment_mass'] - mass.mean()) <= bound.max()
    # the one utterance the figures show: slices of the picked batch
    inputs, targets, outputs = kept[int(got['sample_batch'])]
    u = int(got['sample_index'])
    L, T = int(inputs[5][u]), int(inputs[9][u])
    assert int(got['sample_batch']) == report.pick_batch
    assert np.array_equal(got['alignment_pred'], outputs[4][u, :L, :T].float().cpu().numpy())
    assert np.array_equal(got['alignment_target'], target_alignment_oracle(inputs[2][u].cpu().numpy(), L, T))
    assert np.array_equal(got['mel_pred'], outputs[3][0][u, :, :T].float().cpu().numpy())
    assert np.array_equal(got['mel_target'], targets[3][u, :, :T].cpu().numpy())
    assert np.array_equal(got['duration_pred'], outputs[2][0][u, :L].float().cpu().numpy())
    assert np.array_equal(got['pitch_target'], targets[2][u, :L].cpu().numpy())


def test_train_leaves_the_report_and_its_scalars(golden_dir, tmp_path):
    ''' one iteration of `train()` on the golden feature files with a validation after it: `validation/iter_0000001.npz`, the new
        keys in the validation record of `metrics.jsonl`, figures when matplotlib is there '''
    import json
    import os
    from daft_exprt.train import train
    from daft_exprt.validation_report import MODULES
    fx = np.load(os.path.join(golden_dir, 'data_loader.npz'))
    cwd = os.getcwd()
    out = str(tmp_path)
    hp = make_hparams(training_files=os.path.join(golden_dir, 'train_list.txt'), validation_files=os.path.join(golden_dir, 'train_list.txt'),
                      output_directory=out, batch_size=2, accumulation_steps=1, nb_iterations=1, iters_per_checkpoint=1,
                      iters_check_for_model_improvement=1)
    for cfg in (hp.prosody_encoder, hp.phoneme_encoder, hp.frame_decoder):
        cfg['nb_blocks'] = 2
    hp.stats = {f'spk {i}': {'energy': {'mean': float(fx['stats_energy_mean'][i]), 'std': float(fx['stats_energy_std'][i])},
                             'pitch': {'mean': float(fx['stats_pitch_mean'][i]), 'std': float(fx['stats_pitch_std'][i])}} for i in range(11)}
    hp.rank, hp.world_size, hp.multiprocessing_distributed = 0, 1, False
    os.chdir(golden_dir)
    try:
        train(0, hp, os.path.join(out, 'logs', 'train.log'))
    finally:
        os.chdir(cwd)
    recs = [json.loads(line) for line in open(os.path.join(out, 'logs', 'metrics.jsonl'))]
    val = [r for r in recs if 'DaftExprt.validation/loss' in r]
    assert len(val) == 1 and val[0]['iteration'] == 1
    new = [k for k in val[0] if k.startswith('DaftExprt.film/') or 'alignment' in k]
    assert 0. <= val[0]['DaftExprt.validation/alignment_hit_rate'] <= 1. and 0. < val[0]['DaftExprt.validation/alignment_mass'] <= 1.
    assert len(new) == 2 + 4 * (2 + 1 + 2)
    for m, nb in zip(MODULES, (2, 1, 2)):
        for blk in range(nb):
            assert np.isfinite([val[0][f'DaftExprt.film/{m}/block{blk}/{name}_{stat}'] for name in ('gamma', 'beta') for stat in ('mean', 'std')]).all()
    got = np.load(os.path.join(out, 'validation', 'iter_0000001.npz'))
    n_val = sum(1 for line in open(os.path.join(golden_dir, 'train_list.txt')) if line.strip())
    assert got['alignment_frames'].shape == (n_val,) and got['film_decoder_counts'].shape == (2, 2, BINS)
    assert (got['film_encoder_counts'].sum(-1) == n_val * hp.phoneme_encoder['hidden_embed_dim']).all()     # every utterance, last partial batch included
    assert got['alignment_pred'].shape == got['alignment_target'].shape
    pngs = [f for f in os.listdir(os.path.join(out, 'validation')) if f.endswith('.png')]
    try:
        import matplotlib  # noqa: F401
        assert len(pngs) == 11
    except ImportError:
        assert not pngs


def test_benchmark_sentences_are_generated_beside_their_reference(tmp_path):
    ''' `generate_benchmark_sentences` end to end: a tone as the validation utterance's recording, two phonemised sentences; the
        reference's parameters, one mel-spectrogram and one Griffin-Lim wav per sentence and a copy of the reference wav land in the
        output directory, the draws come from Random(seed + iteration) and the model is back in training mode '''
    import os
    import random
    from daft_exprt import audio
    from daft_exprt.model import DaftExprt
    from daft_exprt.train import generate_benchmark_sentences
    from tests import pitch_cases as PC
    hp = make_hparams(speakers=['spkA', 'spkB'], validation_files=str(tmp_path / 'validation.txt'))
    for cfg in (hp.prosody_encoder, hp.phoneme_encoder, hp.frame_decoder):
        cfg['nb_blocks'] = 2
    hp.stats = {f'spk {i}': {'pitch': {'mean': 5.0, 'std': 0.3}} for i in range(2)}
    hp.data_set_dir, hp.benchmark_dir = str(tmp_path / 'data'), str(tmp_path / 'benchmark')
    sr = int(hp.sampling_rate)
    t = np.arange(int(0.6 * sr)) / sr
    os.makedirs(tmp_path / 'data' / 'spkB' / 'wavs')
    wav = str(tmp_path / 'data' / 'spkB' / 'wavs' / 'utt7.wav')
    audio.write_wav_int16(wav, sr, np.round(PC.harmonic_tone(130.0 + 60.0 * t / t[-1], sr, 0.6) * 32767.0).astype(np.int16))
    (tmp_path / 'validation.txt').write_text(f'{tmp_path}/features/spkB|utt7|1\n')
    os.makedirs(tmp_path / 'benchmark' / 'english')
    (tmp_path / 'benchmark' / 'english' / 'sentences_phonemised.txt').write_text('hello|{HH AH0 L OW1} {W ER1 L D} . ~\ntest|{T EH1 S T} ~\n')
    torch.manual_seed(1234)
    model = DaftExprt(hp)
    with torch.no_grad():   # random duration head: centre it so that the utterances have a sensible length
        model.prosody_predictor.projection.linear_layer.weight[0].mul_(0.05)
        model.prosody_predictor.projection.linear_layer.bias.copy_(torch.tensor([0.08, 0., 0.]))
    model = model.to(DEV).train()
    out = str(tmp_path / 'checkpoints' / 'chk_3')
    preds = generate_benchmark_sentences(model, hp, out, 3)
    assert model.training
    spk = random.Random(hp.seed + 3).choice(hp.speakers_id)
    assert sorted(preds) == [f'hello_spk_{spk}_ref_utt7', f'test_spk_{spk}_ref_utt7']
    assert sorted(os.listdir(out)) == sorted([f'{n}.{ext}' for n in list(preds) + ['utt7'] for ext in ('npz', 'wav')])
    assert open(os.path.join(out, 'utt7.wav'), 'rb').read() == open(wav, 'rb').read()
    for name, pred in preds.items():
        assert pred[4].shape[0] == 80 and pred[4].shape[1] > 0 and np.isfinite(pred[4]).all()
        assert os.path.getsize(os.path.join(out, f'{name}.wav')) > 44
