"""Phoneme boundaries of a recording by dynamic time warping against the model's own synthesis of the same text.

The reference starts from the `.markers` files of an external forced aligner; this module writes them instead.  A trained
checkpoint synthesises the phonemised sentence with the recording itself as prosody reference (as `evaluate.copy_synthesis`
does), the model returns the integer frame count it gave each symbol, the mel cepstra of synthesis and recording are aligned by
the DTW of csrc/dtw_eval.hip, and csrc/align.hip carries the symbol durations over the path (`dx_dtw_transfer`) after
`dx_active_span` has trimmed the silence around the recording.  `markers_from_durations` turns the result into the rows
`begin end phone word word_idx` that `extract_features` reads, `align_data_set` does it for the recordings of a data set and
`scripts/align.py` is its command line.

How close such boundaries come to a trained aligner's on real speech has not been measured.  What is pinned is the
arithmetic: the kernels are integer-exact against tests/align_oracle.py, known boundaries of constructed warps are recovered
exactly, and the rows written pass through `extract_features` with one row per phone.  `moved` (how many boundaries the
minimum-duration repair had to shift) and the mean cost along the path are reported per file so that a user can look at the
worst files first.  No CPU fallback: without the HIP library / a GPU the device functions raise.
"""
import json
import logging
import os
import time
from types import SimpleNamespace

import numpy as np
import torch

from daft_exprt import _hip as H
from daft_exprt.evaluate import dtw_align_batch, max_dtw_length, mel_cepstrum_batch
from daft_exprt.extract_features import sentence_tokens
from daft_exprt.generate import _symbol_ids, read_phonemised_sentences
from daft_exprt.recordings import ALIGN_KEYS, _parameters_of, active_span_batch, copy_inference, empty_alignment  # noqa: F401
from daft_exprt.recordings import load_recordings, pad_references, phonemised_by_speaker, sounding_crops, write_early_statuses
from daft_exprt.symbols import SIL_PHONE_SYMBOL, SIL_WORD_SYMBOL, punctuation
from daft_exprt.write_behind import WriteBehind

_logger = logging.getLogger(__name__)

STATUS = {0: 'ok', 1: 'the recording has fewer frames than its sounding symbols need',
          2: 'the synthesis gave nothing to transfer', 3: 'longer than the DTW takes',
          4: 'the sounding stretch is shorter than the analysis window'}


def dtw_transfer_batch(path, path_len, n_ref, n_gen, gen_durations, n_symbols, min_frames):
    ''' `dx_dtw_transfer`: path (B, T_ref + T_gen - 1, 2) / path_len (B,) int32 as `evaluate.dtw_align_batch` returns them
        (i: the recording, n_ref frames; j: the synthesis, n_gen frames), gen_durations (B, L) int64: the frames of every symbol
        in the synthesis, n_symbols (B,) int64.  Returns (rec_durations (B, L) int64, moved (B,) int32, status (B,) int32): the
        frames of every symbol in the recording, at least min_frames for a symbol that has frames in the synthesis; how many
        starts the repair moved; 0 ok, 1 n_ref < min_frames * sounding symbols, 2 nothing to transfer. '''
    H.require_gpu(path, path_len, n_ref, n_gen, gen_durations, n_symbols)
    assert path.dtype == torch.int32 and path_len.dtype == torch.int32 and path.dim() == 3 and path.shape[2] == 2 and path.is_contiguous()
    assert n_ref.dtype == torch.int64 and n_gen.dtype == torch.int64 and n_symbols.dtype == torch.int64
    assert gen_durations.dtype == torch.int64 and gen_durations.dim() == 2 and gen_durations.is_contiguous()
    B, L = gen_durations.shape
    assert path.shape[0] == B and path_len.shape == (B,) and n_ref.shape == (B,) and n_gen.shape == (B,) and n_symbols.shape == (B,)
    # the kernel is told the extents the path was laid out for; their sum is what matters, so any split that holds the longest
    # row of either side will do (one read-back; `transfer_durations` knows the extents and reads nothing back)
    T_ref = max(1, int(n_ref.max()), path.shape[1] + 1 - max_dtw_length())
    T_gen = path.shape[1] + 1 - T_ref
    if T_gen < max(1, int(n_gen.max())):
        raise ValueError(f'a path of {path.shape[1]} entries per pair cannot hold {int(n_ref.max())} x {int(n_gen.max())} frames')
    return _transfer(path, path_len, n_ref, n_gen, gen_durations, n_symbols, min_frames, T_ref, T_gen)


def _transfer(path, path_len, n_ref, n_gen, gen_durations, n_symbols, min_frames, T_ref, T_gen):
    B, L = gen_durations.shape
    assert T_ref >= 1 and T_gen >= 1 and T_ref + T_gen - 1 == path.shape[1]
    dev = path.device
    rec = torch.empty((B, L), dtype=torch.int64, device=dev)
    moved = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    H.check(H.lib().dx_dtw_transfer(H.ptr(path), H.ptr(path_len.contiguous()), H.ptr(n_ref.contiguous()), H.ptr(n_gen.contiguous()),
                                    H.ptr(gen_durations), H.ptr(n_symbols.contiguous()), H.ptr(rec), H.ptr(moved), H.ptr(status), B,
                                    T_ref, T_gen, L, int(min_frames), H.stream()))
    return rec, moved, status


def _transfer_from_mels(mel_gen, n_gen, gen_durations, n_symbols, mel_rec, n_rec, min_frames, n_coeffs):
    cep_rec = mel_cepstrum_batch(mel_rec, n_rec, n_coeffs)
    cep_gen = mel_cepstrum_batch(mel_gen, n_gen, n_coeffs)
    total, path, path_len = dtw_align_batch(cep_rec, n_rec, cep_gen, n_gen)
    rec, moved, status = _transfer(path, path_len, n_rec, n_gen, gen_durations.contiguous(), n_symbols, min_frames,
                                   mel_rec.shape[2], mel_gen.shape[2])
    return rec, moved, status, total, path_len


def transfer_durations(mel_gen, n_gen, gen_durations, n_symbols, mel_rec, n_rec, min_frames=3, n_coeffs=13):
    ''' mel_gen (B, n_mel, T_gen) / mel_rec (B, n_mel, T_rec) fp32 natural-log mels on the device with n_gen / n_rec (B,) int64
        frames; gen_durations (B, L) int64: the frames of each symbol in mel_gen, n_symbols (B,) int64.  Cepstra of both sides,
        their DTW with the recording on the reference axis, the transfer: returns (rec_durations (B, L) int64, moved (B,) int32,
        status (B,) int32, total (B,) fp32: the accumulated cost of the path).  No model is involved. '''
    H.require_gpu(mel_gen, n_gen, gen_durations, n_symbols, mel_rec, n_rec)
    return _transfer_from_mels(mel_gen, n_gen, gen_durations, n_symbols, mel_rec, n_rec, min_frames, n_coeffs)[:4]


def align_batch(model, symbols, input_lengths, wavs, n_samples, speaker_ids, hparams, min_frames=3, trim_db=-40.0):
    ''' symbols (B, L) / input_lengths (B,) / speaker_ids (B,) int64 and wavs (B, S) fp32 at hparams.sampling_rate on the device,
        n_samples: the B sample counts on the host.  Per utterance: the mel front-end's frame energies give the sounding stretch
        [begin, end) (`recordings.sounding_crops`, trim_db below the peak), the recording is cropped to it, the crop's energy, pitch
        and mel are both the prosody reference of a free-running synthesis (`recordings.copy_inference`, as
        `evaluate.copy_synthesis`) and the target its mel is warped onto (`transfer_durations`).  Returns {key: (B,) device tensor,
        the durations (B, L)} for ALIGN_KEYS, rows in the caller's order:
          begin          first frame of the crop in the recording (int64);  frames: the crop's frames;  frames_gen: the synthesis'
          rec_durations  frames of every symbol in the crop, summing to `frames` where status is 0 (int64)
          gen_durations  frames the model gave every symbol in its synthesis (int64)
          moved, status  as `dtw_transfer_batch`, and status 3: more than `evaluate.max_dtw_length()` frames (the recording's:
                         decided before any launch; the synthesis': before the DTW), 4: a recording or a sounding stretch of no
                         more than filter_length / 2 samples.  rec_durations and moved are 0 where status != 0.
          path_cost      the DTW total divided by the path length (fp32; NaN where status is 3 or 4) '''
    H.require_gpu(symbols, input_lengths, wavs, speaker_ids)
    dev = wavs.device
    B, L = symbols.shape
    out = empty_alignment(B, L, dev)
    with torch.no_grad():
        status, rows, begin, cropped, lengths, _ = sounding_crops(wavs, n_samples, hparams, trim_db)
        if rows:
            idx = torch.tensor(rows, dtype=torch.int64, device=dev)
            energy_refs, pitch_refs, mel_rec, n_rec = pad_references(_parameters_of(cropped, lengths, hparams), dev)
            enc, (mel_gen, n_gen), _, _ = copy_inference(model, symbols[idx], input_lengths[idx], energy_refs, pitch_refs, mel_rec, n_rec,
                                                         speaker_ids[idx], hparams)
            mel_gen, n_gen = mel_gen.float().contiguous(), n_gen.long().contiguous()
            gen_dur = torch.zeros((len(rows), L), dtype=torch.int64, device=dev)
            gen_dur[:, :enc[1].shape[1]] = enc[1].long()
            # a synthesis longer than the DTW takes: status 3 as well
            long_rows = [i for i, n in enumerate(n_gen.tolist()) if n > max_dtw_length()]
            for i in long_rows:
                status[rows[i]] = 3
            fit = [i for i in range(len(rows)) if i not in set(long_rows)]
            if fit:
                sel = torch.tensor(fit, dtype=torch.int64, device=dev)
                n_gen_fit = n_gen[sel].contiguous()
                mel_gen_fit = mel_gen[sel][:, :, :max(int(n_gen_fit.max()), 1)].contiguous()
                rec, moved, st, total, path_len = _transfer_from_mels(mel_gen_fit, n_gen_fit, gen_dur[sel].contiguous(),
                                                                      input_lengths[idx][sel].contiguous(), mel_rec[sel].contiguous(),
                                                                      n_rec[sel].contiguous(), min_frames, 13)
                to = idx[sel]
                out['rec_durations'][to], out['moved'][to], out['status'][to] = rec, moved, st
                out['gen_durations'][to] = gen_dur[sel]
                out['path_cost'][to] = total / path_len.clamp(min=1).float()
                out['begin'][to] = torch.tensor([begin[i] for i in fit], dtype=torch.int64, device=dev)
                out['frames'][to], out['frames_gen'][to] = n_rec[sel], n_gen_fit
    write_early_statuses(out, status)
    return out


# ---- from frame counts to the rows of a .markers file (host) ----------------------------------------------------------------------

def flatten_sentence(sentence):
    ''' [(symbol, index of its word or None)] of a phonemised sentence -- words as lists of phones, boundary symbols as strings
        (`generate.read_phonemised_sentences`) -- one entry per symbol id the model is given, in order '''
    flat, word = [], 0
    for item in sentence:
        if isinstance(item, (list, tuple)):
            flat.extend((phone, word) for phone in item)
            word += 1
        else:
            flat.append((item, None))
    return flat


def lab_words(lab_sentence):
    ''' the words of a .lab sentence as `extract_features.update_markers` will look for them in the markers '''
    return [token for token in sentence_tokens(lab_sentence)[0] if token not in punctuation]


def boundary_time(frame, begin_frame, n_samples, hparams):
    ''' '%.6f' seconds of boundary `frame` (in frames of the crop that starts at begin_frame): half a hop in front of the
        frame's centre, inside the recording -- the grid on which `extract_features` gives every row back its frames '''
    sample = min(max((begin_frame + frame - 0.5) * int(hparams.hop_length), 0.0), float(n_samples))
    return '%.6f' % (sample / float(hparams.sampling_rate))


def markers_from_durations(sentence, words, rec_durations, begin_frame, n_samples, hparams):
    ''' sentence: the phonemised sentence; words: `lab_words` of the utterance's .lab sentence; rec_durations: the frames of every
        symbol (`flatten_sentence` order) in the crop that starts at frame begin_frame of a recording of n_samples.  Returns the
        lines `begin\\tend\\tphone\\tword\\tword_idx\\n` of a .markers file: one per phone, with its word and its word's index; the
        symbols with frames between two words become one `SIL` / `<sil>` row with an index of its own; those in front of the
        first word and behind the last one (closing punctuation, eos) are left out, their frames fall outside the sentence as an
        aligner's trimmed silence does.  A row ends where the next one begins, to the character (`boundary_time`).
        None when the words are not as many as the sentence's brace groups, or when a phone has no frames. '''
    flat = flatten_sentence(sentence)
    durations = [int(d) for d in rec_durations]
    n_words = sum(isinstance(item, (list, tuple)) for item in sentence)
    if len(durations) != len(flat) or len(words) != n_words or n_words == 0:
        return None
    if any(d <= 0 for (_, word), d in zip(flat, durations) if word is not None):
        return None
    edges = np.concatenate([[0], np.cumsum(durations)]).tolist()
    first = next(s for s, (_, word) in enumerate(flat) if word is not None)
    last = max(s for s, (_, word) in enumerate(flat) if word is not None)
    rows, group, idx, s = [], None, -1, first
    while s <= last:
        symbol, word = flat[s]
        if word is not None:
            row, mine, after = (edges[s], edges[s + 1], symbol, word), ('word', word), s + 1
        else:
            after = s
            while flat[after][1] is None:     # (ends at a phone: `last` is one)
                after += 1
            row, mine = (edges[s], edges[after], SIL_PHONE_SYMBOL, None), ('sil', s)
        if row[1] > row[0]:
            if mine != group:                 # every word and every silence is a group of rows with an index of its own
                group, idx = mine, idx + 1
            rows.append(row + (idx,))
        s = after
    stamp = {e: boundary_time(e, begin_frame, n_samples, hparams) for row in rows for e in row[:2]}
    return [f'{stamp[b]}\t{stamp[e]}\t{phone}\t{SIL_WORD_SYMBOL if word is None else words[word]}\t{i}\n' for b, e, phone, word, i in rows]


# ---- a data set -----------------------------------------------------------------------------------------------------------------------

class _MarkerFiles(object):
    ''' `write` of the pass's `WriteBehind`: formats and writes the .markers of one batch and keeps the records of the report '''
    def __init__(self, dataset_dir, hparams, records, skipped):
        self.dataset_dir, self.hparams, self.records, self.skipped = dataset_dir, hparams, records, skipped

    def __call__(self, raw, layout, utts):
        parts, off = {}, 0
        for key, dtype, shape in layout:
            size = int(np.prod(shape)) * np.dtype(dtype).itemsize
            parts[key] = raw[off: off + size].view(dtype).reshape(shape)
            off += size
        for b, u in enumerate(utts):
            status, n_sym = int(parts['status'][b]), len(flatten_sentence(u.sentence))
            cost = float(parts['path_cost'][b])
            record = {'status': status, 'moved': int(parts['moved'][b]), 'path_cost': cost if np.isfinite(cost) else None,
                      'frames': int(parts['frames'][b]), 'frames_gen': int(parts['frames_gen'][b]), 'symbols': n_sym}
            self.records[f'{u.speaker}/{u.name}'] = record
            reason = None
            if status != 0:
                reason = STATUS[status]
            else:
                lines = markers_from_durations(u.sentence, u.words, parts['rec_durations'][b, :n_sym].tolist(), int(parts['begin'][b]),
                                               u.n_samples, self.hparams)
                if lines is None:
                    reason = 'a phone of a word got no frames'
            if reason is not None:
                _logger.warning(f'Ignoring {u.speaker} -- {u.name} -- {reason}')
                self.skipped.append((u.speaker, u.name, reason))
                record['written'] = False
                continue
            with open(os.path.join(self.dataset_dir, u.speaker, 'align', f'{u.name}.markers'), 'w', encoding='utf-8') as f:
                f.write(''.join(lines))
            record['written'] = True


def _summary(records):
    done = [r for r in records.values() if r['written']]
    costs = [r['path_cost'] for r in done if r['path_cost'] is not None]
    return {'files': len(records), 'written': len(done),
            'status': {str(k): sum(r['status'] == k for r in records.values()) for k in sorted(STATUS)},
            'moved_total': sum(r['moved'] for r in done), 'files_with_moved': sum(r['moved'] > 0 for r in done),
            'moved_per_symbol': (sum(r['moved'] for r in done) / max(1, sum(r['symbols'] for r in done))),
            'mean_path_cost': float(np.mean(costs)) if costs else None, 'max_path_cost': float(np.max(costs)) if costs else None}


def align_data_set(dataset_dir, speakers, phonemised_files, model, hparams, batch_size=32, min_frames=3, trim_db=-40.0,
                   overwrite=False, report_file=None, device='cuda:0'):
    ''' model: a `DaftExprt` (its synthesis is warped onto the recording, `align_batch`) or an `aligner.Aligner` (its learned
        alignment, `Aligner.align_batch`: any speaker name goes, `frames_gen` is then the symbol count and `path_cost` the negative
        MAS score per frame).
        for every speaker -- `<dataset_dir>/<speaker>/wavs/NAME.wav`, `<dataset_dir>/<speaker>/align/NAME.lab` and the `NAME|...`
        lines of the speaker's phonemised file (`generate.read_phonemised_sentences`; phonemised_files: {speaker: path}, a list
        in the order of `speakers`, or one path for all) -- writes `<dataset_dir>/<speaker>/align/NAME.markers` from
        `align_batch`, batch_size utterances at a time: the wavs go to the device through `recordings.load_recordings`, the results come
        back through `write_behind.WriteBehind`.  Existing .markers are kept unless `overwrite`.  The speaker id is the one
        `hparams.speakers_id` holds for the speaker.  An utterance without a wav or a .lab, whose .lab words are not as many as
        its phonemised words, or that ends with status != 0 or a phone without frames is skipped with a warning.
        Returns the report and writes it to report_file (default `<dataset_dir>/align_report.json`): {'files': {'speaker/NAME':
        {status, moved, path_cost, frames, frames_gen, symbols, written}}, 'summary': {...}, 'skipped': [[speaker, NAME, reason]],
        'already_done', 'batches', 'seconds', 'min_frames', 'trim_db'}. '''
    from daft_exprt.aligner import Aligner     # (`aligner` imports this module for `dtw_transfer_batch`)
    dev = H.device(device)
    fs = int(hparams.sampling_rate)
    speakers = list(speakers)
    learned = isinstance(model, Aligner)     # a learned aligner knows no speakers: any name goes, the id is unused
    run = model.align_batch if learned else (lambda *a: align_batch(model, *a))
    phonemised_files = phonemised_by_speaker(phonemised_files, speakers)
    records, skipped = {}, []
    report = {'files': records, 'summary': {}, 'skipped': skipped, 'already_done': 0, 'batches': 0, 'seconds': 0.,
              'min_frames': int(min_frames), 'trim_db': float(trim_db)}
    start = time.time()
    for speaker in speakers:
        if not learned and speaker not in hparams.speakers:
            raise ValueError(f'speaker "{speaker}" is not one of the model\'s: {hparams.speakers}')
        speaker_id = 0 if learned else int(hparams.speakers_id[hparams.speakers.index(speaker)])
        wavs_dir, align_dir = os.path.join(dataset_dir, speaker, 'wavs'), os.path.join(dataset_dir, speaker, 'align')
        for path in (wavs_dir, align_dir):
            if not os.path.isdir(path):
                raise FileNotFoundError(f'There is no such directory: {path}')
        sentences, names = read_phonemised_sentences(phonemised_files[speaker], hparams.symbols)
        todo = []
        for sentence, name in zip(sentences, names):
            wav_file, lab_file = os.path.join(wavs_dir, f'{name}.wav'), os.path.join(align_dir, f'{name}.lab')
            if os.path.isfile(os.path.join(align_dir, f'{name}.markers')) and not overwrite:
                report['already_done'] += 1
                continue
            missing = [what for what, path in (('wav', wav_file), ('.lab', lab_file)) if not os.path.isfile(path)]
            if missing:
                _logger.warning(f'Ignoring {speaker} -- {name} -- no {missing[0]} file')
                skipped.append((speaker, name, f'no {missing[0]} file'))
                continue
            with open(lab_file, 'r', encoding='utf-8') as f:
                words = lab_words(f.readline())
            if len(words) != sum(isinstance(item, (list, tuple)) for item in sentence):
                _logger.warning(f'Ignoring {speaker} -- {name} -- the .lab sentence and the phonemised sentence differ in their words')
                skipped.append((speaker, name, 'the .lab sentence and the phonemised sentence differ in their words'))
                continue
            todo.append(SimpleNamespace(speaker=speaker, name=name, sentence=sentence, words=words, wav_file=wav_file,
                                        ids=_symbol_ids(sentence, hparams)))
        writer = WriteBehind(_MarkerFiles(dataset_dir, hparams, records, skipped), 'markers_writer')
        try:
            for pos in range(0, len(todo), int(batch_size)):
                utts = todo[pos: pos + int(batch_size)]
                symbols, (input_lengths, speaker_ids), wavs, n_total = load_recordings(utts, fs, dev, [(speaker_id,)] * len(utts))
                out = run(symbols, input_lengths, wavs, n_total, speaker_ids, hparams, min_frames, trim_db)
                named = [(key, out[key]) for key in ALIGN_KEYS]
                layout = [(key, str(t.dtype).replace('torch.', ''), tuple(t.shape)) for key, t in named]
                writer.put(torch.cat([t.contiguous().view(-1).view(torch.uint8) for _, t in named]), layout, utts)
                report['batches'] += 1
        finally:
            writer.close()
    report['seconds'] = time.time() - start
    report['summary'] = _summary(records)
    report_file = os.path.join(dataset_dir, 'align_report.json') if report_file is None else report_file
    with open(report_file, 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=1)
    s = report['summary']
    _logger.info(f'{s["written"]} of {s["files"]} files aligned, {len(skipped)} skipped, {report["already_done"]} already done -- '
                 f'{s["moved_total"]} starts moved in {s["files_with_moved"]} files -- report: {report_file}')
    return report
