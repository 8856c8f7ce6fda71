"""Prosody cloning: a recording's timing, loudness and intonation, symbol by symbol, imposed on a synthesis.

The reference lets a recording act as the utterance-level prosody reference and lets the predictor's outputs be scaled by factors.
This module adds targets in absolute terms: `ProsodyTargets` holds, per symbol, a duration in frames, an energy and a pitch (any
of the three may be absent) and a weight in [0, 1] for each; `DaftExprt.inference(..., prosody_targets=...)` imposes them on the
predictor's outputs (`dx_prosody_impose`, csrc/prosody_targets.hip) in front of the factors, the integer durations and the pitch
transform.  Where a whole row is given in frames at weight 1, the integer durations ARE the targets (`dx_prosody_impose_durations`):
the synthesis is frame-synchronous with the recording ("frame-exact").

`targets_from_recordings` makes the targets of a batch of recordings of the same sentences: the phoneme boundaries come from
`align.align_batch` (the checkpoint's own synthesis) or `Aligner.align_batch` (a learned aligner, 9l), the per-symbol
energies and pitches from `dx_clone_pool` over the front-end's frame curves.  `clone_batch` runs the second-pass synthesis with
them, makes audio as `generate.generate_batch_mel_specs` does, and scores the result against the recording frame by frame -- the
identity path through `dx_dtw_path_scores` -- where the row is frame-exact.  `scripts/clone.py` is the command line.

How close cloned speech sounds to the recording on real data has not been measured.  What is pinned is the arithmetic (the kernels
against tests/prosody_targets_oracle.py) and the contract: frame-exact rows come out with the recording's frame counts, rows that
could not be aligned are synthesised free-running and reported, never cloned from zeros.  No CPU fallback: without the HIP library
/ a GPU the device functions raise.
"""
import json
import logging
import math
import os
import time
from types import SimpleNamespace

import numpy as np
import torch

from daft_exprt import _hip as H
from daft_exprt import audio, evaluate, griffin_lim, ops
from daft_exprt.align import STATUS, align_batch
from daft_exprt.extract_features import mel_spectrogram_batch, pitch_batch
from daft_exprt.generate import _symbol_ids
from daft_exprt.recordings import _parameters_of, copy_inference, load_recordings, pad_references, sounding_crops, unwrap
from daft_exprt.vocoder import pcm16

_logger = logging.getLogger(__name__)

QUANTITIES = ('dur', 'energy', 'pitch')
_FIELD = {'dur': 'durations', 'energy': 'energy', 'pitch': 'pitch'}
UNITS = ('standardised', 'raw')
NORMALISE = ('self', 'source', 'target')
SCORE_KEYS = ('mcd_db', 'f0_rmse_cents', 'vuv_error', 'pitch_pcc', 'energy_pcc')
INFO_KEYS = ('status', 'begin', 'frames', 'moved', 'path_cost', 'dropped', 'pool_status', 'usable')


def _check_scalar_weight(name, w):
    if not 0.0 <= float(w) <= 1.0:       # (NaN fails both comparisons)
        raise ValueError(f'ProsodyTargets: {name} = {w} (a weight lies in [0, 1])')


class ProsodyTargets(object):
    ''' Per-symbol prosody targets of a batch, rows in the batch's order.
          durations  (B, L) int64 frames, < 0 where a symbol has no target;  energy, pitch  (B, L) fp32
          w_dur, w_energy, w_pitch   a scalar or (B, L) fp32 in [0, 1]; kept as (B, L) fp32 for the targets given, None otherwise
          units      'standardised': energy and pitch as the model predicts them (`data_loader._standardise` with the statistics
                     of the speaker that will speak);  'raw': energy as the front-end gives it, pitch in natural-log Hz -- turn
                     them into model units with `standardised(hparams, speaker_ids)` before `inference`
        A zero energy / pitch target says "silent" / "unvoiced" (in both units) and is taken over from weight 0.5 on.
        Tensors may live on the host (`permute` and `to` work there); `inference` needs them on the device.
        `validate` checks (B, L) weights against [0, 1], which reads one flag back; scalar weights are checked on the host. '''

    def __init__(self, durations=None, energy=None, pitch=None, w_dur=1.0, w_energy=1.0, w_pitch=1.0, units='standardised',
                 validate=True):
        if units not in UNITS:
            raise ValueError(f'ProsodyTargets: units = {units!r} (one of {UNITS})')
        given = [t for t in (durations, energy, pitch) if t is not None]
        if not given:
            raise ValueError('ProsodyTargets: no target given')
        shape, dev = tuple(given[0].shape), given[0].device
        if len(shape) != 2 or any(tuple(t.shape) != shape or t.device != dev for t in given):
            raise ValueError(f'ProsodyTargets: the targets must share one (B, L) shape and one device, got {[tuple(t.shape) for t in given]}')
        self.units = units
        self.durations = None if durations is None else durations.to(torch.int64).contiguous()
        self.energy = None if energy is None else energy.to(torch.float32).contiguous()
        self.pitch = None if pitch is None else pitch.to(torch.float32).contiguous()
        for name, target, w in (('w_dur', self.durations, w_dur), ('w_energy', self.energy, w_energy), ('w_pitch', self.pitch, w_pitch)):
            if target is None:
                w = None
            elif torch.is_tensor(w):
                if tuple(w.shape) != shape:
                    raise ValueError(f'ProsodyTargets: {name} of shape {tuple(w.shape)} for targets of shape {shape}')
                w = w.to(device=dev, dtype=torch.float32).contiguous()
                if validate and not bool(((w >= 0) & (w <= 1)).all()):
                    raise ValueError(f'ProsodyTargets: {name} has a value outside [0, 1]')
            else:
                _check_scalar_weight(name, w)
                w = torch.full(shape, float(w), dtype=torch.float32, device=dev)
            setattr(self, name, w)

    @property
    def shape(self):
        return tuple(next(t for t in (self.durations, self.energy, self.pitch) if t is not None).shape)

    def _like(self, f):
        ''' a new object whose tensors are f(tensor) '''
        new = object.__new__(ProsodyTargets)
        new.units = self.units
        for key in ('durations', 'energy', 'pitch', 'w_dur', 'w_energy', 'w_pitch'):
            t = getattr(self, key)
            setattr(new, key, None if t is None else f(t).contiguous())
        return new

    def to(self, device):
        return self._like(lambda t: t.to(device))

    def permute(self, order):
        ''' rows `order[0], order[1], ...` of this batch, in that order: the collate's sort by symbol count '''
        order = torch.as_tensor(order, dtype=torch.int64)
        if sorted(order.tolist()) != list(range(self.shape[0])):
            raise ValueError(f'ProsodyTargets.permute: {order.tolist()} is no permutation of {self.shape[0]} rows')
        return self._like(lambda t: t[order.to(t.device)])

    def narrow(self, L):
        ''' the first L symbols of every row '''
        return self._like(lambda t: t[:, :L])

    def select(self, what):
        ''' only the quantities named in `what` (a subset of ('dur', 'energy', 'pitch')) '''
        what = tuple(what)
        unknown = [q for q in what if q not in QUANTITIES]
        if unknown or not what:
            raise ValueError(f'ProsodyTargets.select: {what} (a non-empty subset of {QUANTITIES})')
        new = self._like(lambda t: t)
        for q, w in zip(QUANTITIES, ('w_dur', 'w_energy', 'w_pitch')):
            if q not in what:
                setattr(new, _FIELD[q], None)
                setattr(new, w, None)
        return new

    def scaled(self, weights):
        ''' every weight multiplied by a scalar in [0, 1], or by {'dur' / 'energy' / 'pitch': scalar} '''
        factors = weights if isinstance(weights, dict) else {q: weights for q in QUANTITIES}
        new = self._like(lambda t: t)
        for q, name in zip(QUANTITIES, ('w_dur', 'w_energy', 'w_pitch')):
            f = float(factors.get(q, 1.0))
            _check_scalar_weight(f'weights[{q!r}]', f)
            w = getattr(new, name)
            if w is not None and f != 1.0:
                setattr(new, name, w * f)
        return new

    def masked(self, keep):
        ''' weight 0 everywhere in the rows where `keep` ((B,) bool) is False '''
        new = self._like(lambda t: t)
        for name in ('w_dur', 'w_energy', 'w_pitch'):
            w = getattr(new, name)
            if w is not None:
                setattr(new, name, torch.where(keep.to(w.device)[:, None], w, torch.zeros_like(w)))
        return new

    def standardised(self, hparams, speaker_ids):
        ''' these targets in model units for the speakers that will speak: raw energies and natural-log-Hz pitches go through
            `data_loader._standardise` with the statistics of speaker_ids (B host ints), zeros staying zeros.  Standardised
            targets are returned as they are. '''
        if self.units == 'standardised':
            return self
        ids = [int(s) for s in (speaker_ids.tolist() if torch.is_tensor(speaker_ids) else speaker_ids)]
        if len(ids) != self.shape[0]:
            raise ValueError(f'ProsodyTargets.standardised: {len(ids)} speaker ids for {self.shape[0]} rows')
        new = self._like(lambda t: t)
        new.units = 'standardised'
        for key in ('energy', 'pitch'):
            t = getattr(new, key)
            if t is not None:
                mean, std = _speaker_stats(hparams, ids, key, t.device)
                setattr(new, key, torch.where(t == 0, torch.zeros_like(t), (t - mean[:, None]) / std[:, None]))
        return new

    @staticmethod
    def stack(items, L, device=None):
        ''' one batch from per-sentence targets: items[b] is None (no target: weight 0 everywhere) or a ProsodyTargets of one row
            with at most L symbols; a quantity absent from an item gets weight 0 in its row.  None when every item is None. '''
        present = [it for it in items if it is not None]
        if not present:
            return None
        units = {it.units for it in present}
        if len(units) != 1:
            raise ValueError('ProsodyTargets.stack: the items mix standardised and raw units')
        dev = next(t for t in (present[0].durations, present[0].energy, present[0].pitch) if t is not None).device if device is None else device
        B = len(items)
        out = {}
        for key, w, dtype, fill in (('durations', 'w_dur', torch.int64, -1), ('energy', 'w_energy', torch.float32, 0.), ('pitch', 'w_pitch', torch.float32, 0.)):
            if all(getattr(it, key) is None for it in present):
                continue
            target, weight = torch.full((B, L), fill, dtype=dtype), torch.zeros((B, L), dtype=torch.float32)
            for b, it in enumerate(items):
                if it is None or getattr(it, key) is None:
                    continue
                if it.shape[0] != 1 or it.shape[1] > L:
                    raise ValueError(f'ProsodyTargets.stack: item {b} has shape {it.shape}, expected one row of at most {L} symbols')
                n = it.shape[1]
                target[b, :n], weight[b, :n] = getattr(it, key)[0].cpu(), getattr(it, w)[0].cpu()
            out[key], out[w] = target.to(dev), weight.to(dev)
        return ProsodyTargets(units=units.pop(), validate=False, **out)


def _speaker_stats(hparams, speaker_ids, feature, device):
    ''' (mean, std) (B,) fp32 on the device of hparams.stats for the speakers; KeyError for a speaker without statistics '''
    rows = [hparams.stats[f'spk {int(s)}'][feature] for s in speaker_ids]
    mean = torch.tensor([float(r['mean']) for r in rows], dtype=torch.float32)
    std = torch.tensor([float(r['std']) for r in rows], dtype=torch.float32)
    return mean.to(device), std.to(device)


def _align(obj, *args):
    return obj.align_batch(*args) if hasattr(obj, 'align_batch') else align_batch(obj, *args)


def targets_from_recordings(aligner_or_model, symbols, input_lengths, wavs, n_samples, speaker_ids, hparams, normalise='self',
                            target_speaker_ids=None, min_frames=3, trim_db=-40.0):
    ''' symbols (B, L) / input_lengths (B,) / speaker_ids (B,) int64 and wavs (B, S) fp32 at hparams.sampling_rate on the device,
        n_samples: the B sample counts on the host -- recordings of the sentences, by the speakers speaker_ids.
        The phoneme boundaries are `aligner_or_model`'s: `align.align_batch` for a `DaftExprt`, its own `align_batch` for an
        `aligner.Aligner`.  The per-symbol energies and pitches are pooled by `dx_clone_pool` from the front-end's curves of the
        WHOLE recording, starting at the sounding stretch's first frame, and standardised with
          normalise = 'self'    the utterance's own statistics: the contour relative to the recording itself
                      'source'  the recorded speaker's entry in hparams.stats: the contour relative to that speaker
                      'target'  the entry of target_speaker_ids ((B,) host ints or a tensor): the same Hz in the target's units
        Returns (targets, info).  targets: a `ProsodyTargets` (standardised units, weight 1) with the durations in frames, the
        energies and the pitches; rows that were not aligned (status != 0) or not pooled have weight 0 everywhere, and a quantity
        whose statistics could not be used (`dropped`) has weight 0 in its row: such rows are synthesised free-running.
        info: {status, begin, frames, moved, path_cost: as `align.align_batch`; dropped (B,) int32 and self_stats (B, 4) fp32 as
        `dx_clone_pool`, pool_status (B,) int32; energy_refs, pitch_refs (B, T) fp32, mel (B, n_mel, T) fp32, n_rec (B,) int64: the
        sounding stretch analysed on its own, i.e. the recording as utterance-level prosody reference -- for a row with status != 0
        the whole recording, untrimmed, with zeros behind it up to one analysis window: a reference to synthesise it free-running
        with; usable (B,) bool: the rows whose targets carry weight}. '''
    if normalise not in NORMALISE:
        raise ValueError(f'normalise = {normalise!r} (one of {NORMALISE})')
    if normalise == 'target' and target_speaker_ids is None:
        raise ValueError("normalise='target' needs target_speaker_ids")
    H.require_gpu(symbols, input_lengths, wavs, speaker_ids)
    dev = wavs.device
    B, L = symbols.shape
    n_samples = [int(n) for n in (n_samples.tolist() if torch.is_tensor(n_samples) else n_samples)]
    with torch.no_grad():
        out = _align(aligner_or_model, symbols, input_lengths, wavs, n_samples, speaker_ids, hparams, min_frames, trim_db)
        status = out['status'].cpu().tolist()
        rows = [b for b in range(B) if status[b] == 0]
        sym_energy = torch.zeros((B, L), dtype=torch.float32, device=dev)
        sym_pitch = torch.zeros((B, L), dtype=torch.float32, device=dev)
        self_stats = torch.zeros((B, 4), dtype=torch.float32, device=dev)
        dropped = torch.zeros((B,), dtype=torch.int32, device=dev)
        pool_status = torch.zeros((B,), dtype=torch.int32, device=dev)
        info = {key: out[key] for key in ('status', 'begin', 'frames', 'moved', 'path_cost')}
        refs = {}
        if rows:
            idx = torch.tensor(rows, dtype=torch.int64, device=dev)
            sub_n = [n_samples[b] for b in rows]
            n_dev = torch.tensor(sub_n, dtype=torch.int64, device=dev)
            sub = wavs[idx][:, :max(sub_n)].contiguous()
            # the curves of the whole recording: the front-end's frame energies and the pitch track, frame for frame
            _, energy, n_frames = mel_spectrogram_batch(sub, n_dev, hparams, min_samples=min(sub_n))
            log_pitch, _ = pitch_batch(sub, n_dev, hparams)
            T = min(energy.shape[1], log_pitch.shape[1])
            stats = {'self': None, 'source': [int(s) for s in speaker_ids[idx].tolist()] if normalise == 'source' else None,
                     'target': [int(target_speaker_ids[b]) for b in rows] if normalise == 'target' else None}[normalise]
            pairs = (None, None) if stats is None else tuple(_speaker_stats(hparams, stats, f, dev) for f in ('energy', 'pitch'))
            e, p, ss, dr, ps = ops.clone_pool(energy[:, :T], log_pitch[:, :T], out['begin'][idx].contiguous(),
                                              out['rec_durations'][idx].contiguous(), input_lengths[idx].contiguous(), pairs[0], pairs[1])
            sym_energy[idx], sym_pitch[idx], self_stats[idx], dropped[idx], pool_status[idx] = e, p, ss, dr, ps
            # the sounding stretch on its own, as `align_batch` analysed it (the same front end on these energies): the utterance's reference
            _, kept, _, cropped, lengths, _ = sounding_crops(sub, sub_n, hparams, trim_db, energy, n_frames)
            if kept:
                refs = dict(zip([rows[i] for i in kept], _parameters_of(cropped, lengths, hparams)))
        # a row that was not aligned still needs a reference to be synthesised free-running: its whole recording, untrimmed, with
        # zeros behind it up to one analysis window where it is shorter than that
        rest = [b for b in range(B) if b not in refs]
        if rest:
            lengths = [max(n_samples[b], int(hparams.filter_length)) for b in rest]
            whole = torch.zeros((len(rest), max(lengths)), dtype=torch.float32, device=dev)
            for i, b in enumerate(rest):
                whole[i, :n_samples[b]] = wavs[b, :n_samples[b]]
            refs.update(zip(rest, _parameters_of(whole, lengths, hparams)))
        energy_refs, pitch_refs, mel, n_rec = pad_references([refs[b] for b in range(B)], dev)
        info.update(energy_refs=energy_refs, pitch_refs=pitch_refs, mel=mel, n_rec=n_rec, dropped=dropped, self_stats=self_stats,
                    pool_status=pool_status)
        usable = (out['status'] == 0) & (pool_status == 0) & (info['n_rec'] == out['frames'])
        ones = usable[:, None].expand(B, L).to(torch.float32)
        targets = ProsodyTargets(durations=out['rec_durations'], energy=sym_energy, pitch=sym_pitch, w_dur=ones.clone(),
                                 w_energy=ones * ((dropped & 1) == 0)[:, None], w_pitch=ones * ((dropped & 2) == 0)[:, None],
                                 validate=False)
        info['usable'] = usable
    return targets, info


def _identity_path(n, T_ref, T_gen, device):
    ''' path (B, T_ref + T_gen - 1, 2) int32 / path_len (B,) int32 as `dx_dtw_align` lays them out: the cells (i, i), i < n[b] '''
    P = T_ref + T_gen - 1
    i = torch.arange(P, dtype=torch.int32, device=device)[None, :, None]
    path = torch.where(i < n.to(torch.int32)[:, None, None], i, torch.full_like(i, -1)).expand(n.shape[0], P, 2).contiguous()
    return path, n.to(torch.int32).contiguous()


def clone_batch(model, symbols, input_lengths, wavs, n_samples, speaker_ids, target_speaker_ids, hparams, aligner=None,
                what=QUANTITIES, weights=1.0, normalise='self', vocoder=None, use_griffin_lim=False, min_frames=3, trim_db=-40.0,
                seconds=None):
    ''' The sentences symbols (B, L) / input_lengths (B,), spoken by target_speaker_ids (B,) int64, with the prosody of the
        recordings wavs (B, S) fp32 / n_samples (host) of the same sentences by speaker_ids -- all tensors on the device.
        `targets_from_recordings` (through `aligner` when one is given, else through `model` itself), then ONE second-pass
        `inference` with the targets of the quantities in `what`, their weights scaled by `weights` (a scalar or a dict per
        quantity), the recording's sounding stretch as utterance-level reference, factors 1 and pitch transform 'add' 0.  Audio is
        made as `generate.generate_batch_mel_specs` makes it: `vocoder`'s, else the Griffin-Lim preview with `use_griffin_lim`, else
        none.  A row that could not be aligned is synthesised free-running, with its whole recording as reference.
        Returns rows in the caller's order, tensors on the device:
          mel (B, n_mel, T) fp32, n_frames (B,) int64, dur_int (B, L) int64, energy, pitch, dur (B, L) fp32: what `inference` returns
          wavs (B, S') fp32, n_samples (B,) int64: the audio, or None
          frame_exact (B,) bool: the row's integer durations are the recording's
          scores {key: (B,) fp32} for SCORE_KEYS, NaN where undefined:
            mcd_db         the cloned mel against the sounding stretch's mel, frame against frame (the identity path through
                           `dx_mel_cepstrum` / `dx_dtw_path_scores`): defined for frame-exact rows only
            f0_rmse_cents, vuv_error   the pitch track of the generated audio against the recording's, same path (audio only)
            pitch_pcc, energy_pcc      `evaluate.prosody_transfer_scores` of the generated audio (audio only, aligned rows only)
          targets, info: as `targets_from_recordings` returns them (targets before `what` / `weights`).
        seconds: a dict that receives the wall time of the stages 'alignment + pooling', 'second pass', 'audio + scores' (each ends
        with a device synchronisation, so pass it only to measure). '''
    H.require_gpu(symbols, input_lengths, wavs, speaker_ids, target_speaker_ids)
    dev = wavs.device
    B, L = symbols.shape

    def lap(name, begin):
        if seconds is not None:
            torch.cuda.synchronize(dev)
            seconds[name] = seconds.get(name, 0.) + time.time() - begin
        return time.time()

    clock = time.time()
    targets, info = targets_from_recordings(aligner if aligner is not None else model, symbols, input_lengths, wavs, n_samples,
                                            speaker_ids, hparams, normalise, target_speaker_ids.tolist() if normalise == 'target' else None,
                                            min_frames, trim_db)
    clock = lap('alignment + pooling', clock)
    imposed = targets.select(what).scaled(weights)
    with torch.no_grad():
        enc, (mel, n_frames), _, order = copy_inference(model, symbols, input_lengths, info['energy_refs'], info['pitch_refs'], info['mel'],
                                                        info['n_rec'], target_speaker_ids, hparams, prosody_targets=imposed)
        exact = unwrap(model).last_frame_exact                    # (in the order `inference` saw the rows in)
        exact = ((exact if order is None else exact[torch.argsort(order)]) == 1) & info['usable']
        mel, n_frames = mel.float().contiguous(), n_frames.long().contiguous()
        wide = lambda t, dtype: torch.cat([t.to(dtype), torch.zeros((B, L - t.shape[1]), dtype=dtype, device=dev)], dim=1)
        result = {'mel': mel, 'n_frames': n_frames, 'dur': wide(enc[0], torch.float32), 'dur_int': wide(enc[1], torch.int64),
                  'energy': wide(enc[2], torch.float32), 'pitch': wide(enc[3], torch.float32), 'frame_exact': exact,
                  'targets': targets, 'info': info, 'wavs': None, 'n_samples': None}
        clock = lap('second pass', clock)

        nan = torch.full((B,), float('nan'), dtype=torch.float32, device=dev)
        scores = {key: nan.clone() for key in SCORE_KEYS}
        T_rec, T_gen = info['mel'].shape[2], mel.shape[2]
        if max(T_rec, T_gen) <= evaluate.max_dtw_length():
            cep_rec = evaluate.mel_cepstrum_batch(info['mel'], info['n_rec'])
            cep_gen = evaluate.mel_cepstrum_batch(mel, n_frames)
            both = torch.where(exact, torch.minimum(info['n_rec'], n_frames), torch.zeros_like(n_frames))
            path, path_len = _identity_path(both, T_rec, T_gen, dev)
            scores['mcd_db'] = evaluate.dtw_path_scores_batch(cep_rec, info['n_rec'], cep_gen, n_frames, path, path_len)[0]
        if vocoder is not None:
            vocoder.check_hparams(hparams)
            audio, n_audio = vocoder(mel, n_frames)
        elif use_griffin_lim:
            audio, n_audio = griffin_lim.griffin_lim_batch(mel, n_frames, hparams)
        else:
            audio = None
        if audio is not None:
            result['wavs'], result['n_samples'] = audio, n_audio
            pcc = evaluate.prosody_transfer_scores(audio, n_audio, info['pitch_refs'], info['energy_refs'], info['n_rec'], hparams)
            for key in ('pitch_pcc', 'energy_pcc'):
                scores[key] = torch.where(info['usable'], pcc[key], nan)
            if max(T_rec, T_gen) <= evaluate.max_dtw_length():
                lp_gen, n_lp = pitch_batch(audio, n_audio, hparams)
                if lp_gen.shape[1] < T_gen:
                    lp_gen = torch.cat([lp_gen, torch.zeros((B, T_gen - lp_gen.shape[1]), dtype=torch.float32, device=dev)], dim=1)
                path, path_len = _identity_path(torch.minimum(both, n_lp.long()), T_rec, T_gen, dev)
                _, f0, vuv, _, _ = evaluate.dtw_path_scores_batch(cep_rec, info['n_rec'], cep_gen, n_frames, path, path_len,
                                                                  info['pitch_refs'].contiguous(), lp_gen.contiguous())
                scores['f0_rmse_cents'], scores['vuv_error'] = f0, vuv
        result['scores'] = scores
        lap('audio + scores', clock)
    return result


# ---- the report (host) ------------------------------------------------------------------------------------------------------------

def _number(x):
    x = float(x)
    return x if math.isfinite(x) else None


def clone_report(names, host):
    ''' names: the B file names; host: {key: B host values} for INFO_KEYS, 'frame_exact' and SCORE_KEYS (lists or NumPy arrays).
        Returns {'files': {name: {status, frames, begin, moved, path_cost, dropped, pool_status, usable, frame_exact, scores: {...}}},
        'summary': {'files', 'status': {status: count}, 'usable': count, 'frame_exact': count, 'scores': {key: {'mean', 'files'}}}}.
        `usable` false says the file was synthesised free-running; the reason is `status` (the alignment's), else `pool_status` 1 (the
        aligned rows overran the recording's curves), else the re-analysed sounding stretch had another frame count than the
        alignment's `frames`.  NaN is written as null, the means run over the files where the score is defined. '''
    files = {}
    for b, name in enumerate(names):
        files[name] = {'status': int(host['status'][b]), 'frames': int(host['frames'][b]), 'begin': int(host['begin'][b]),
                       'moved': int(host['moved'][b]), 'path_cost': _number(host['path_cost'][b]), 'dropped': int(host['dropped'][b]),
                       'pool_status': int(host['pool_status'][b]), 'usable': bool(host['usable'][b]),
                       'frame_exact': bool(host['frame_exact'][b]), 'scores': {key: _number(host[key][b]) for key in SCORE_KEYS}}
    summary = {'files': len(files), 'status': {str(k): sum(f['status'] == k for f in files.values()) for k in sorted(STATUS)},
               'usable': sum(f['usable'] for f in files.values()), 'frame_exact': sum(f['frame_exact'] for f in files.values()),
               'scores': {}}
    for key in SCORE_KEYS:
        values = [f['scores'][key] for f in files.values() if f['scores'][key] is not None]
        summary['scores'][key] = {'mean': float(np.mean(values)) if values else None, 'files': len(values)}
    return {'files': files, 'summary': summary}


def merge_reports(reports):
    ''' one report from the reports of several batches (file names are unique across them) '''
    files = {}
    for r in reports:
        files.update(r['files'])
    host = {key: [f[key] if key in f else f['scores'][key] for f in files.values()] for key in INFO_KEYS + ('frame_exact',) + SCORE_KEYS}
    for key in SCORE_KEYS + ('path_cost',):
        host[key] = [float('nan') if v is None else v for v in host[key]]
    return clone_report(list(files), host)


def clone_files(model, sentences, names, wav_files, target_speaker_ids, output_dir, hparams, aligner=None, source_speaker_ids=None,
                what=QUANTITIES, normalise='self', batch_size=32, vocoder=None, use_griffin_lim=True, min_frames=3, trim_db=-40.0,
                device='cuda:0'):
    ''' sentences / names as `generate.read_phonemised_sentences` returns them, wav_files: one recording (any rate) per sentence,
        target_speaker_ids: one id per sentence; source_speaker_ids: the recorded speakers (default: the targets; they matter to
        the synthesis-based alignment and to normalise='source').  batch_size sentences at a time through `clone_batch`; writes
        `<output_dir>/<name>.npz` (key mel_spec) and `<name>.wav` as `generate.generate_batch_mel_specs` does (the vocoder's audio
        as 16-bit PCM, the Griffin-Lim preview as 64-bit float) and `<output_dir>/clone_report.json` (`clone_report`).  Returns
        the report. '''
    dev = H.device(device)
    fs = int(hparams.sampling_rate)
    n = len(sentences)
    source_speaker_ids = list(target_speaker_ids) if source_speaker_ids is None else list(source_speaker_ids)
    for what_, seq in (('names', names), ('recordings', wav_files), ('target speakers', target_speaker_ids), ('source speakers', source_speaker_ids)):
        if len(seq) != n:
            raise ValueError(f'{len(seq)} {what_} for {n} sentences')
    os.makedirs(output_dir, exist_ok=True)
    reports = []
    for pos in range(0, n, int(batch_size)):
        sl = slice(pos, pos + int(batch_size))
        utts = [SimpleNamespace(wav_file=path, ids=_symbol_ids(s, hparams)) for path, s in zip(wav_files[sl], sentences[sl])]
        symbols, (input_lengths, source, target), wavs, n_total = load_recordings(utts, fs, dev, list(zip(source_speaker_ids[sl],
                                                                                                         target_speaker_ids[sl])))
        out = clone_batch(model, symbols, input_lengths, wavs, n_total, source, target, hparams, aligner=aligner, what=what,
                          normalise=normalise, vocoder=vocoder, use_griffin_lim=use_griffin_lim and vocoder is None, min_frames=min_frames,
                          trim_db=trim_db)
        host = {key: out['info'][key].cpu().numpy() for key in INFO_KEYS}
        host['frame_exact'] = out['frame_exact'].cpu().numpy()
        host.update({key: out['scores'][key].cpu().numpy() for key in SCORE_KEYS})
        mel, n_frames = out['mel'].cpu().numpy(), out['n_frames'].cpu().numpy()
        if out['wavs'] is not None:
            samples = (pcm16(out['wavs']) if vocoder is not None else out['wavs']).cpu().numpy()
            n_out = out['n_samples'].cpu().numpy()
            write = audio.write_wav_int16 if vocoder is not None else audio.write_wav
        for b, name in enumerate(names[sl]):
            np.savez(os.path.join(output_dir, f'{name}.npz'), mel_spec=mel[b, :, :int(n_frames[b])])
            if out['wavs'] is not None:
                write(os.path.join(output_dir, f'{name}.wav'), fs, samples[b, :int(n_out[b])])
        reports.append(clone_report(names[sl], host))
    report = merge_reports(reports)
    report.update(what=list(what), normalise=normalise, audio='hifi-gan' if vocoder is not None else 'griffin-lim' if use_griffin_lim else None,
                  aligner='learned' if aligner is not None else 'synthesis')
    with open(os.path.join(output_dir, 'clone_report.json'), 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=1)
    s = report['summary']
    _logger.info(f'{s["frame_exact"]} of {s["files"]} files cloned frame-exact -- statuses {s["status"]} -- report: '
                 f'{os.path.join(output_dir, "clone_report.json")}')
    return report
