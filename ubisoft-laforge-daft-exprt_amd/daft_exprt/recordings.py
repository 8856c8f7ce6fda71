"""What relates a recording to its text, stated once for `align`, `aligner`, `clone`, `evaluate` and `generate`: a
sounding stretch as a crop, the front end of the aligners and of cloning, the result of both `align_batch`, reference triples as
batch tensors, copy inference, the walk over a data set.  Imports only `audio`, `extract_features` and `_hip`.  No CPU fallback."""
import os

import numpy as np
import torch

from daft_exprt import _hip as H
from daft_exprt import audio
from daft_exprt.extract_features import mel_spectrogram_batch, nb_frames, pitch_batch, wav_crop_batch


def max_dtw_length():
    ''' longest sequence (frames) `evaluate.dtw_align_batch` and the lattices of `aligner` take '''
    return int(H.lib().dx_dtw_max_len())


def _take(t, rows):     # rows `rows` (ascending, distinct) of t: t itself when they are all of its rows
    return t if len(rows) == t.shape[0] else t[torch.tensor(rows, dtype=torch.int64, device=t.device)]


def early_statuses(n_samples, hparams):
    ''' per recording of n_samples (host ints), before any launch: 3 with more frames than `max_dtw_length()`, 4 with no more than
        filter_length / 2 samples (the front end's reflect padding needs more), else 0 '''
    limit, half = max_dtw_length(), int(hparams.filter_length) // 2
    return [3 if nb_frames(n, hparams) > limit else 4 if n <= half else 0 for n in n_samples]


def span_crops(spans, n_samples, hop_length, filter_length):
    ''' spans: per row the sounding stretch (begin_frame, end_frame) of a recording of n_samples -> per row (begin_frame, first_sample,
        n_crop_samples), cut at hop multiples with the end inside the recording, or status 4 where that is <= filter_length / 2 samples '''
    hop, half = int(hop_length), int(filter_length) // 2
    crops = [(f0, f0 * hop, min(f1 * hop, n) - f0 * hop) for (f0, f1), n in zip(spans, n_samples)]
    return [4 if c[2] <= half else c for c in crops]


def active_span_batch(energy, n_frames, rel_db=-40.0):
    ''' `dx_active_span`: energy (B, T) fp32 and n_frames (B,) int64 on the device -> (begin, end) (B,) int64: the first frame
        whose energy reaches the row's peak * 10^(rel_db / 20) and one past the last; (0, 0) for an empty or all-zero row '''
    H.require_gpu(energy, n_frames)
    assert energy.dtype == torch.float32 and energy.dim() == 2 and energy.stride(1) == 1 and n_frames.dtype == torch.int64
    B, T = energy.shape
    assert n_frames.shape == (B,)
    begin, end = (torch.empty((B,), dtype=torch.int64, device=energy.device) for _ in range(2))
    H.check(H.lib().dx_active_span(H.ptr(energy), energy.stride(0), H.ptr(n_frames.contiguous()), float(rel_db), H.ptr(begin),
                                   H.ptr(end), B, T, H.stream()))
    return begin, end


def sounding_crops(wavs, n_samples, hparams, trim_db, energy=None, n_frames=None):
    ''' wavs (B, S) fp32 at hparams.sampling_rate on the device, n_samples: the B sample counts on the host.  Per recording the
        sounding stretch of the frame energies (`active_span_batch`, trim_db below the peak), cut out at hop multiples.  energy (B, T)
        fp32 / n_frames (B,) int64: the front end's frame energies of `wavs` if the caller has them, else they are computed here.
        Returns (status: B host ints, 3 / 4 as `early_statuses` and `span_crops` say, else 0;  rows: the b with status 0, and for those
        begin: the crop's first frame in the recording;  cropped (len(rows), max(lengths)) fp32: the crops, zeros behind them;  lengths:
        their samples, host ints;  crop (len(rows), 2) int64 on the device: first sample, samples -- the last three None without rows) '''
    if not hparams.centered:
        raise ValueError('sounding_crops: the frames [begin, end) are cut at hop multiples only with hparams.centered')
    n_samples = [int(n) for n in (n_samples.tolist() if torch.is_tensor(n_samples) else n_samples)]
    status = early_statuses(n_samples, hparams)
    rows = [b for b in range(len(n_samples)) if status[b] == 0]
    if not rows:
        return status, [], [], None, None, None
    sub_n = [n_samples[b] for b in rows]
    sub = _take(wavs, rows)[:, :max(sub_n)].contiguous()
    if energy is None:
        _, energy, n_frames = mel_spectrogram_batch(sub, torch.tensor(sub_n, dtype=torch.int64, device=sub.device), hparams, min_samples=min(sub_n))
    else:
        energy, n_frames = _take(energy, rows), _take(n_frames, rows)
    begin, end = active_span_batch(energy, n_frames, trim_db)
    crops = span_crops(torch.stack([begin, end], dim=1).cpu().tolist(), sub_n, hparams.hop_length, hparams.filter_length)
    keep = [i for i, c in enumerate(crops) if c != 4]
    for i, b in enumerate(rows):
        status[b] = 0 if i in keep else 4
    if not keep:
        return status, [], [], None, None, None
    crops = [crops[i] for i in keep]
    lengths = [c[2] for c in crops]
    crop = torch.tensor([[c[1], c[2]] for c in crops], dtype=torch.int64, device=sub.device)
    cropped = wav_crop_batch(_take(sub, keep).contiguous(), crop, max(lengths))
    return status, [rows[i] for i in keep], [c[0] for c in crops], cropped, lengths, crop


ALIGN_KEYS = ('begin', 'rec_durations', 'gen_durations', 'moved', 'status', 'path_cost', 'frames', 'frames_gen')


def empty_alignment(B, L, device):
    ''' the dict of ALIGN_KEYS for B rows of L symbols in which nothing is aligned yet: zeros, path_cost NaN '''
    out = {key: torch.zeros((B, L) if key.endswith('_durations') else (B,), dtype=torch.int32 if key in ('moved', 'status') else torch.int64,
                            device=device) for key in ALIGN_KEYS}
    out['path_cost'] = torch.full((B,), float('nan'), dtype=torch.float32, device=device)
    return out


def write_early_statuses(out, status):
    ''' status: B host ints; those that are not 0 -- decided on the host -- go into out['status'] '''
    early = [b for b, s in enumerate(status) if s != 0]
    if early:
        out['status'][torch.tensor(early, device=out['status'].device)] = torch.tensor([status[b] for b in early], dtype=torch.int32,
                                                                                       device=out['status'].device)


def _parameters_of(wavs, lengths, hparams):
    ''' [(energy (T,), pitch (T,), mel_spec (n_mel, T)) NumPy] of the (B, S) fp32 device waveforms `wavs` at
        hparams.sampling_rate, zeros past their `lengths` (host ints): one `pitch_batch` and one `mel_spectrogram_batch` '''
    n = torch.tensor(lengths, dtype=torch.int64, device=wavs.device)
    pitch, n_pitch = pitch_batch(wavs, n, hparams)
    mel, energy, n_mel = mel_spectrogram_batch(wavs, n, hparams)
    pitch, energy, mel, n_pitch, n_mel = (t.cpu().numpy() for t in (pitch, energy, mel, n_pitch, n_mel))
    out = []
    for i in range(len(lengths)):
        t = int(n_mel[i])
        assert int(n_pitch[i]) == t, f'{int(n_pitch[i])} -- {t}'            # `generate.py:459`
        out.append((energy[i, :t].copy(), pitch[i, :t].copy(), mel[i, :, :t].copy()))
    return out


def pad_references(triples, device):
    ''' [(energy (T_b,), pitch (T_b,), mel (n_mel, T_b)) NumPy], one per row -> (energy_refs, pitch_refs (B, T) fp32, mel
        (B, n_mel, T) fp32, n_rec (B,) int64) on the device: T the longest row, zeros behind every row, n_rec the T_b '''
    B, T = len(triples), max(m.shape[1] for _, _, m in triples)
    energy_refs, pitch_refs = np.zeros((B, T), dtype=np.float32), np.zeros((B, T), dtype=np.float32)
    mel = np.zeros((B, triples[0][2].shape[0], T), dtype=np.float32)
    for b, (e, p, m) in enumerate(triples):
        energy_refs[b, :len(e)], pitch_refs[b, :len(p)], mel[b, :, :m.shape[1]] = e, p, m
    n_rec = np.array([m.shape[1] for _, _, m in triples], dtype=np.int64)
    return tuple(torch.from_numpy(a).to(device) for a in (energy_refs, pitch_refs, mel, n_rec))


def unwrap(model):
    ''' the `DaftExprt` of a model that may be wrapped (DDP: `.module`) '''
    return model if hasattr(model, 'inference') else model.module


def copy_inference(model, symbols, input_lengths, energy_refs, pitch_refs, mel, n_rec, speaker_ids, hparams, prosody_targets=None):
    ''' the free-running synthesis of symbols (B, L) / input_lengths (B,) by speaker_ids (B,) with the prosody references energy_refs,
        pitch_refs (B, T), mel (B, n_mel, T), n_rec (B,) -- a recording as its own reference: copy synthesis --, factors 1 and pitch
        transform 'add' with factor 0; tensors on the device, rows in any order.  `inference` takes its batches longest first, as the
        collates sort them: the rows, and those of prosody_targets (a `clone.ProsodyTargets`), are sorted so (stable) for it.  The
        model (DDP-wrapped or not) runs in eval mode, without gradients, and goes back to the mode it was in.  Returns (encoder_preds,
        (mel, n_frames), alignments, order): as `inference` returns them but rows in the caller's order, and the permutation
        (sorted = x[order]; None for a batch the sort leaves in place) '''
    core = unwrap(model)
    with torch.no_grad():
        lens, order = torch.sort(input_lengths, descending=True, stable=True)
        if order.tolist() == list(range(len(order))):
            order = None
        width = max(int(lens[0]), 1)
        sort = (lambda t: t) if order is None else (lambda t: t[order])
        sym = sort(symbols)[:, :width].contiguous()
        ones = torch.ones(sym.shape, dtype=torch.float32, device=sym.device)
        targets = prosody_targets if prosody_targets is None or order is None else prosody_targets.permute(order.cpu())
        kw = {} if targets is None else {'prosody_targets': targets.narrow(width)}
        refs = (sort(t).contiguous() for t in (energy_refs, pitch_refs, mel, n_rec, speaker_ids))
        was_training = core.training
        core.eval()
        enc, (mel_gen, n_gen), alignments = core.inference((sym, ones, ones, torch.zeros_like(ones), lens.contiguous(), *refs), 'add',
                                                           hparams, **kw)
        core.train(was_training)
        if order is not None:
            back = torch.argsort(order)
            enc, mel_gen, n_gen, alignments = tuple(t[back] for t in enc), mel_gen[back], n_gen[back], alignments[back]
    return enc, (mel_gen, n_gen), alignments, order


def phonemised_by_speaker(phonemised_files, speakers):
    ''' {speaker: path} of phonemised_files: such a dict, a list in the order of `speakers`, or one path for all '''
    if isinstance(phonemised_files, dict):
        return phonemised_files
    if isinstance(phonemised_files, (str, os.PathLike)):
        phonemised_files = [phonemised_files] * len(speakers)
    assert len(phonemised_files) == len(speakers), f'{len(phonemised_files)} phonemised files for {len(speakers)} speakers'
    return dict(zip(speakers, phonemised_files))


def waves_to_device(utts, fs, device):
    ''' utts: records with `.wav_file` (any rate): read on the host, brought to fs on the device (`audio.device_waves`); every
        record gets `.rate` and `.n_samples`, the host samples are released.  Returns (wavs (B, S) fp32, the B sample counts). '''
    for u in utts:
        x, u.rate = audio.read_wav(u.wav_file)
        u.samples = audio.to_float_mono(x)
    wavs, n_total = audio.device_waves(utts, fs, device)
    for u, n in zip(utts, n_total):
        u.n_samples, u.samples = n, None
    return wavs, n_total


def load_recordings(utts, fs, device, ints=None):
    ''' utts: records with `.wav_file` and `.ids` (symbol ids); ints: further host ints per record.  `waves_to_device`, the padded ids,
        and every row's symbol count and ints in one copy -> (symbols (B, L), [input_lengths, *ints], wavs) on the device, n_samples '''
    wavs, n_total = waves_to_device(utts, fs, device)
    symbols = torch.zeros((len(utts), max(len(u.ids) for u in utts)), dtype=torch.int64)
    for b, u in enumerate(utts):
        symbols[b, :len(u.ids)] = torch.tensor(u.ids, dtype=torch.int64)
    rows = [[len(u.ids)] + [int(i) for i in (ints[b] if ints is not None else ())] for b, u in enumerate(utts)]
    columns = torch.tensor(rows, dtype=torch.int64).to(device)
    return symbols.to(device), [columns[:, k].contiguous() for k in range(columns.shape[1])], wavs, n_total
