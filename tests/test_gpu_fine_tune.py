"""GPU checks of the vocoder fine-tuning data set: `dx_resample` against the float64 oracle (tests/resample_oracle.py), equal-rate
pass-through, ragged batches, `dx_ft_pack`, and `fine_tuning` end to end on a data set fabricated in tmp_path."""
import os

import numpy as np
import pytest
import torch

from oracle import daft_exprt_cpu as O
from oracle.fill import fill_params
from tests import resample_oracle as RO
from tests.util import make_hparams

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def _signals(n, seed):
    rng = np.random.RandomState(seed)
    noise = rng.uniform(-1, 1, size=n)
    t = np.arange(n) / n
    chirp = np.clip(0.9 * np.sin(2 * np.pi * (50 + 4000 * t) * t * n / 16000.) + 0.2 * rng.randn(n), -1, 1)
    return [noise.astype(np.float32), chirp.astype(np.float32)]


def _resample_dev(xs, sr_in, sr_out):
    from daft_exprt.audio import resample_batch
    S = max(len(x) for x in xs)
    host = np.zeros((len(xs), S), dtype=np.float32)
    for i, x in enumerate(xs):
        host[i, :len(x)] = x
    n = torch.tensor([len(x) for x in xs], dtype=torch.int64, device=DEV)
    y, n_out = resample_batch(torch.from_numpy(host).to(DEV), n, sr_in, sr_out)
    torch.cuda.synchronize()
    return y.cpu().numpy(), n_out.cpu().numpy()


@pytest.mark.parametrize('sr_in,sr_out', [(16000, 22050), (24000, 22050), (44100, 22050), (48000, 22050), (22050, 16000)])
def test_resample_matches_oracle(sr_in, sr_out):
    xs = _signals(2400, sr_in) + _signals(1700, sr_in + 1)[:1]
    y, n_out = _resample_dev(xs, sr_in, sr_out)
    assert y.shape[1] == RO.out_lengths(2400, sr_in, sr_out)[1]
    worst = 0.
    for i, x in enumerate(xs):
        ref = RO.resample(x, sr_in, sr_out)
        assert n_out[i] == len(ref)
        err = np.abs(y[i, :len(ref)] - ref).max()
        worst = max(worst, err)
        assert not y[i, len(ref):].any()
    print(f'{sr_in} -> {sr_out}: max abs error {worst:.3g}')
    assert worst <= 1e-5


def test_equal_rates_pass_through():
    xs = _signals(3000, 5) + [np.array([0.25, -1., 1.], dtype=np.float32)]
    y, n_out = _resample_dev(xs, 22050, 22050)
    assert y.shape[1] == 3000 and list(n_out) == [3000, 3000, 3]
    for i, x in enumerate(xs):
        assert np.array_equal(y[i, :len(x)], x) and not y[i, len(x):].any()


@pytest.mark.parametrize('sr_in', [16000, 48000])
def test_ragged_batch_is_bit_equal_to_each_alone(sr_in):
    rng = np.random.RandomState(sr_in)
    lengths = [3001, 5, 777, 60, 1400]                   # 5 and 60: shorter than the filter's half-width
    xs = [rng.uniform(-1, 1, size=n).astype(np.float32) for n in lengths]
    y, n_out = _resample_dev(xs, sr_in, 22050)
    for i, x in enumerate(xs):
        alone, n1 = _resample_dev([x], sr_in, 22050)
        assert n_out[i] == n1[0] == RO.out_lengths(len(x), sr_in, 22050)[1]
        assert np.array_equal(y[i, :n1[0]], alone[0, :n1[0]]), i
        assert not y[i, n1[0]:].any()
    small = RO.resample(xs[1], sr_in, 22050)
    assert np.abs(y[1, :len(small)] - small).max() <= 1e-5


def test_ft_pack_crops_packs_and_saturates():
    from daft_exprt.audio import ft_pack
    rng = np.random.RandomState(7)
    B, n_mel, T, S = 3, 80, 50, 700
    mel = rng.randn(B, n_mel, T).astype(np.float32)
    lengths = [50, 17, 33]
    wav = rng.uniform(-1, 1, size=(B, S)).astype(np.float32)
    wav[0, :8] = [1.0, -1.0, 1.5, -1.5, 0.99999, -0.99999, np.nan, -1.0000001]
    wav[1, 100:104] = [3e-5, -3e-5, 0.5 / 32768, -1.5 / 32768]
    crop = [(0, 400), (100, 0), (150, 550)]
    buf = ft_pack(torch.from_numpy(mel).to(DEV), torch.tensor(lengths, device=DEV), torch.from_numpy(wav).to(DEV),
                  torch.tensor(crop, dtype=torch.int64, device=DEV), n_mel * sum(lengths), sum(n for _, n in crop))
    raw = buf.cpu().numpy()
    assert raw.size == 4 * n_mel * sum(lengths) + 2 * sum(n for _, n in crop)
    mels = raw[:4 * n_mel * sum(lengths)].view(np.float32)
    wavs = raw[4 * n_mel * sum(lengths):].view(np.int16)
    mo = wo = 0
    for b in range(B):
        np.testing.assert_array_equal(mels[mo: mo + n_mel * lengths[b]].reshape(n_mel, lengths[b]), mel[b, :, :lengths[b]])
        mo += n_mel * lengths[b]
        begin, n = crop[b]
        w = wav[b, begin:begin + n] * np.float32(32768.)
        expect = np.clip(np.trunc(np.nan_to_num(w, nan=0.)), -32768, 32767).astype(np.int16)
        np.testing.assert_array_equal(wavs[wo: wo + n], expect)
        wo += n
    assert list(wavs[:8]) == [32767, -32768, 32767, -32768, 32767, -32767, 0, -32768]


# ---- end to end -----------------------------------------------------------------------------------------------------------

FS, HOP = 22050, 256


def _write_floats(path, values):
    with open(path, 'w', encoding='utf-8') as f:
        f.write('\n'.join(f'{v:.6f}' for v in values) + '\n')


def _markers(begin, end, durations, hp, rng):
    ''' rows `begin end int_dur symbol word word_idx`; phone boundaries from the integer durations, the last ends at `end` '''
    t, rows = begin, []
    for i, d in enumerate(durations):
        stop = end if i == len(durations) - 1 else t + d * HOP / FS
        rows.append(f'{t:.10f}\t{stop:.10f}\t{d}\t{hp.symbols[int(rng.randint(1, hp.n_symbols))]}\tword\t0')
        t = stop
    return '\n'.join(rows) + '\n'


def _fabricate(tmp_path, hp):
    ''' 2 speakers x 4 utterances; spkB/b1 is stored at 16 kHz, spkA/a3 crops to less than one second.  Returns
        {file: (speaker, expected int16 crop or None, tolerance in LSB)} '''
    from daft_exprt.audio import write_wav_int16
    from daft_exprt.extract_features import mel_spectrogram_HiFi, nb_frames
    rng = np.random.RandomState(3)
    lines, expect = [], {}
    for sid, spk in enumerate(hp.speakers):
        for k in range(4):
            name = f'{spk[-1].lower()}{k}'
            short = name == 'a3'
            T = int(rng.randint(30, 45)) if short else int(rng.randint(95, 140))
            n_c = (T - 1) * HOP + int(rng.randint(0, HOP))
            assert nb_frames(n_c, hp) == T
            a = int(rng.randint(300, 3000))
            e = a + n_c
            n_total = e + int(rng.randint(0, 2000))
            wav_dir, align_dir, feat_dir = (tmp_path / 'data' / spk / 'wavs', tmp_path / 'data' / spk / 'align',
                                            tmp_path / 'features' / spk)
            for d in (wav_dir, align_dir, feat_dir):
                d.mkdir(parents=True, exist_ok=True)
            if name == 'b1':                                   # 16 kHz source: crop of the oracle-resampled signal
                n16 = -(-n_total * 16000 // FS) + 5
                src = np.clip(rng.randn(n16) * 4000, -32768, 32767).astype(np.int16)
                write_wav_int16(str(wav_dir / f'{name}.wav'), 16000, src)
                full = RO.resample(src.astype(np.float64) / 32768., 16000, FS)
                assert len(full) >= e
                crop_f = full[a:e]
                crop16 = np.clip(np.trunc(crop_f.astype(np.float32) * np.float32(32768.)), -32768, 32767).astype(np.int16)
                expect[name] = (spk, crop16, 1)
            else:
                src = np.clip(rng.randn(n_total) * 4000, -32768, 32767).astype(np.int16)
                write_wav_int16(str(wav_dir / f'{name}.wav'), FS, src)
                crop_f = src[a:e].astype(np.float64) / 32768.
                expect[name] = (spk, None if short else src[a:e].copy(), 0)
            if short:
                expect[name] = (spk, None, 0)
            L = int(rng.randint(8, 20))
            dur = np.ones(L, dtype=np.int64)
            for _ in range(T - L):
                dur[rng.randint(0, L)] += 1
            markers = _markers((a + 0.5) / FS, (e + 0.5) / FS, dur, hp, rng)
            (align_dir / f'{name}.markers').write_text(markers, encoding='utf-8')
            (feat_dir / f'{name}.markers').write_text(markers, encoding='utf-8')
            mel = mel_spectrogram_HiFi(crop_f.astype(np.float32), hp)
            assert mel.shape == (hp.n_mel_channels, T)
            np.save(str(feat_dir / f'{name}.npy'), mel)
            base = str(feat_dir / name)
            # the reference's feature ranges: energy = frame L2 norms of exp(mel), pitch = log(f0 in Hz) with 0 where unvoiced
            _write_floats(base + '.symbols_nrg', rng.uniform(2, 30, size=L))
            _write_floats(base + '.symbols_f0', np.log(rng.uniform(90, 250, size=L)))
            _write_floats(base + '.frames_nrg', rng.uniform(0, 40, size=T))
            _write_floats(base + '.frames_f0', np.where(rng.rand(T) < 0.3, 0., np.log(rng.uniform(90, 250, size=T))))
            lines.append(f'{feat_dir}|{name}|{sid}')
    for f in (hp.training_files, hp.validation_files):
        with open(f, 'w', encoding='utf-8') as fh:
            fh.write('\n'.join(lines) + '\n')
    return expect


def _hparams(tmp_path):
    stats = {f'spk {i}': {'energy': {'mean': 15., 'std': 8.}, 'pitch': {'mean': 5., 'std': 0.3}} for i in range(2)}
    (tmp_path / 'exp').mkdir()
    hp = make_hparams(compute_dtype='fp32', speakers=['spkA', 'spkB'], training_files=str(tmp_path / 'exp' / 'train_english.txt'),
                      validation_files=str(tmp_path / 'exp' / 'validation_english.txt'), output_directory=str(tmp_path / 'out'),
                      batch_size=3, stats=stats)
    hp.data_set_dir = str(tmp_path / 'data')
    return hp


def test_fine_tuning_end_to_end(tmp_path, monkeypatch):
    from daft_exprt.audio import read_wav
    from daft_exprt.fine_tune import fine_tuning
    from daft_exprt.model import DaftExprt
    hp = _hparams(tmp_path)
    expect = _fabricate(tmp_path, hp)
    P = fill_params(O.param_shapes(hp))
    ckpt = str(tmp_path / 'DaftExprt_best')
    torch.save({'iteration': 1, 'state_dict': {'module.' + k: v for k, v in P.items()}}, ckpt)
    hp.checkpoint = ckpt
    batches = []                                            # the (shuffled) batches the driver runs, as collated on the host
    parse_batch = DaftExprt.parse_batch

    def recording(self, gpu, batch):
        batches.append((tuple(t.clone() for t in batch[:11]), list(batch[12])))
        return parse_batch(self, gpu, batch)
    monkeypatch.setattr(DaftExprt, 'parse_batch', recording)

    stats = fine_tuning(hp)
    assert stats['utterances'] == 8 and stats['written'] == 7 and stats['skipped'] == 1, stats

    ft = tmp_path / 'exp' / 'fine_tuning_dataset'
    written = sorted(str(p.relative_to(ft)) for p in ft.rglob('*') if p.is_file())
    want = sorted(f'{spk}/{name}.{ext}' for name, (spk, crop, _) in expect.items() if crop is not None for ext in ('npy', 'wav'))
    assert written == want

    # the oracle's teacher-forced eval forward on each of those batches (an utterance's mel depends on the utterances that share
    # its batch, in the oracle as in the kernels, so the comparison is per batch)
    assert len(batches) == 3
    ref_mel = {}
    for b, names in batches:
        f = lambda t: t.float()  # noqa: E731
        i = lambda t: t.long()  # noqa: E731
        cin = (i(b[0]), f(b[1]), i(b[2]), f(b[3]), f(b[4]), i(b[5]), f(b[6]), f(b[7]), f(b[8]), i(b[9]), i(b[10]))
        with torch.no_grad():
            mel = O.forward(P, hp, cin, training=False)[3][0].numpy()
        ref_mel.update({n: mel[r, :, :int(b[9][r])] for r, n in enumerate(names)})
    for name, (spk, crop, lsb) in expect.items():
        if crop is None:
            continue
        ref = ref_mel[name]
        got = np.load(str(ft / spk / f'{name}.npy'))
        assert got.dtype == np.float32 and got.shape == ref.shape
        rel = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12))
        print(f'{name}: written mel vs oracle {rel:.3g}')
        assert rel <= 2e-4, (name, rel)
        x, sr = read_wav(str(ft / spk / f'{name}.wav'))
        assert sr == FS and x.dtype == np.int16 and x.shape == (len(crop), 1)
        diff = np.abs(x[:, 0].astype(np.int32) - crop.astype(np.int32)).max()
        assert diff <= lsb, (name, diff)
        if lsb == 0:
            assert (ft / spk / f'{name}.wav').read_bytes()[44:] == crop.tobytes()

    # a markers span that no longer matches the features' frame count raises and names the file
    m = tmp_path / 'data' / 'spkB' / 'align' / 'b2.markers'
    rows_ = m.read_text(encoding='utf-8').splitlines()
    last = rows_[-1].split('\t')
    last[1] = f'{float(last[1]) - 3 * HOP / FS:.10f}'           # three frames fewer
    rows_[-1] = '\t'.join(last)
    m.write_text('\n'.join(rows_) + '\n', encoding='utf-8')
    with pytest.raises(ValueError, match='b2'):
        fine_tuning(hp)
