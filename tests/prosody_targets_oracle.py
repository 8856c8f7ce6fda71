"""Oracle of the per-symbol prosody-target kernels (csrc/prosody_targets.hip): the contract of include/daft_exprt_hip.h
(K29) in Python integers and float64 NumPy, written from that contract and never from the kernels.
tests/test_prosody_targets_host.py pins it on the CPU (tests/feature_oracle.py's pooling, the loader's `_standardise`,
numpy.mean / numpy.std, hand-built cases); tests/test_gpu_prosody_targets.py holds the kernels and the model to it.

Conventions: "f32(x)" is x rounded once to fp32.  Where the contract fixes the bits (pooled means, statistics, targets at weight 0
and 1, every integer) the oracle returns fp32 / integers to compare with `==`; where it allows fp32 rounding (standardised values,
blended values) it returns float64 and the test states the bound.
"""
import math

import numpy as np

OK, OVERRUN = 0, 1                       # status of dx_clone_pool
ST_EMPTY, ST_WEIGHT = 3, 4               # statuses dx_prosody_impose_durations adds to K16's 1 and 2


def f32(x):
    return np.float32(x)


# ---- dx_clone_pool ------------------------------------------------------------------------------------------------------------------

def pool(energy, log_pitch, begin, durations, T):
    ''' the frames [begin, begin + sum durations) of the curves (their first T frames exist), one stretch per row in order.
        Returns (mean energy, mean of the pitch values > 0 or 0) per row as fp32 -- exact sums, one division in float64, one
        rounding -- or None when begin < 0, a duration is negative or the rows overrun T (nothing may be read then). '''
    durations = [int(d) for d in durations]
    begin = int(begin)
    if begin < 0 or any(d < 0 for d in durations) or begin + sum(durations) > T:
        return None
    energy = np.asarray(energy, dtype=np.float64)[:T]
    log_pitch = np.asarray(log_pitch, dtype=np.float64)[:T]
    sym_energy = np.zeros(len(durations), dtype=np.float32)
    sym_pitch = np.zeros(len(durations), dtype=np.float32)
    frame = begin
    for row, d in enumerate(durations):
        if d == 0:
            continue
        sym_energy[row] = f32(math.fsum(energy[frame: frame + d]) / d)
        voiced = log_pitch[frame: frame + d]
        voiced = voiced[voiced > 0.]
        if len(voiced):
            sym_pitch[row] = f32(math.fsum(voiced) / len(voiced))
        frame += d
    return sym_energy, sym_pitch


def own_stats(values):
    ''' (mean, population std, count) of the non-zero entries of fp32 `values`, in float64, each rounded once to fp32; (0, 0, 0)
        without an entry '''
    v = np.asarray(values, dtype=np.float32)
    v = v[v != 0].astype(np.float64)
    if len(v) == 0:
        return f32(0), f32(0), 0
    mean = math.fsum(v) / len(v)
    var = math.fsum((x - mean) ** 2 for x in v) / len(v)
    return f32(mean), f32(math.sqrt(var)), len(v)


def standardise(values, mean, std):
    ''' float64 (v - mean) / std of the fp32 values with the fp32 statistics, zeros staying exactly 0 '''
    v = np.asarray(values, dtype=np.float32).astype(np.float64)
    out = (v - float(mean)) / float(std)
    out[v == 0] = 0.
    return out


def standardise_bound(values, mean, std):
    ''' what two fp32 roundings (the subtraction, the division) may move a standardised value by: 4 * 2^-24 * (|v| + |mean|) / std '''
    v = np.abs(np.asarray(values, dtype=np.float64))
    return 4 * 2.0 ** -24 * (v + abs(float(mean))) / float(std)


def clone_pool(energy, log_pitch, begin, durations, n_rows, T, L, energy_stats=None, pitch_stats=None):
    ''' one utterance of dx_clone_pool: durations has L entries of which the first n_rows count.  energy_stats / pitch_stats:
        None (the utterance's own) or (mean, std).  Returns a dict: status; raw_energy, raw_pitch (L,) fp32; self_stats (4,) fp32;
        dropped; used (4,) fp32: the statistics applied; sym_energy, sym_pitch (L,) float64. '''
    zeros = lambda dtype: np.zeros(L, dtype=dtype)
    pooled = pool(energy, log_pitch, begin, list(durations)[:int(n_rows)], T)
    if pooled is None:
        return {'status': OVERRUN, 'raw_energy': zeros(np.float32), 'raw_pitch': zeros(np.float32), 'self_stats': np.zeros(4, dtype=np.float32),
                'dropped': 0, 'used': np.zeros(4, dtype=np.float32), 'sym_energy': zeros(np.float64), 'sym_pitch': zeros(np.float64)}
    out = {'status': OK, 'dropped': 0}
    stats, used = [], []
    for bit, (key, raw, given) in enumerate((('energy', pooled[0], energy_stats), ('pitch', pooled[1], pitch_stats))):
        full = zeros(np.float32)
        full[:len(raw)] = raw
        mean, std, count = own_stats(full)
        stats += [mean, std]
        if given is None:
            m, s, drop = mean, std, count < 2 or not std > 0
        else:
            m, s = f32(given[0]), f32(given[1])
            drop = not s > 0
        used += [m, s]
        out[f'raw_{key}'] = full
        out[f'sym_{key}'] = zeros(np.float64) if drop else standardise(full, m, s)
        out['dropped'] |= int(drop) << bit
    out['self_stats'], out['used'] = np.array(stats, dtype=np.float32), np.array(used, dtype=np.float32)
    return out


# ---- dx_prosody_impose / dx_prosody_impose_durations ---------------------------------------------------------------------------------

def target_seconds(frames, hop_length, sampling_rate):
    ''' a duration target in seconds: frames * hop / sampling_rate in float64, rounded once to fp32 '''
    return f32(float(int(frames)) * float(hop_length) / float(sampling_rate))


def blend(x, t, w):
    ''' x moved towards t by w, float64: x + w (t - x).  The contract fixes the bits at w = 0 (x) and w = 1 (t). '''
    x, t, w = float(x), float(t), float(w)
    return x if w == 0 else t if w == 1 else x + w * (t - x)


def blend_level(x, t, w):
    ''' energy / pitch: a zero target says silent / unvoiced and is taken over from w = 0.5 on, ignored below '''
    if float(t) == 0:
        return 0. if float(w) >= 0.5 else float(x)
    return blend(x, t, w)


def blend_bound(x, t):
    ''' the fp32 roundings of t - x and of the fused multiply-add: 2^-23 * (|x| + |t|) '''
    return 2.0 ** -23 * (abs(float(x)) + abs(float(t)))


def _bad(w):
    return not (0 <= float(w) <= 1)


def impose(dur, energy, pitch, length, t_dur=None, t_energy=None, t_pitch=None, w_dur=None, w_energy=None, w_pitch=None,
           dur_factors=None, hop_length=256, sampling_rate=22050):
    ''' one row of dx_prosody_impose.  Returns (dur, energy, pitch as float64 arrays, exact): symbols at or past `length` are
        untouched; exact = -1 (and nothing touched) when a weight that would be used is outside [0, 1]. '''
    out = [np.asarray(a, dtype=np.float32).astype(np.float64).copy() for a in (dur, energy, pitch)]
    n = int(length)
    used = [w[:n] for t, w in ((t_dur, w_dur), (t_energy, w_energy), (t_pitch, w_pitch)) if t is not None]
    if any(_bad(w) for ws in used for w in ws):
        return out[0], out[1], out[2], -1
    exact = int(t_dur is not None and all(int(t_dur[l]) >= 0 and float(w_dur[l]) == 1 and (dur_factors is None or float(dur_factors[l]) == 1)
                                          for l in range(n)))
    for l in range(n):
        if t_dur is not None and int(t_dur[l]) >= 0:
            out[0][l] = blend(out[0][l], target_seconds(t_dur[l], hop_length, sampling_rate), w_dur[l])
        if t_energy is not None:
            out[1][l] = blend_level(out[1][l], f32(t_energy[l]), w_energy[l])
        if t_pitch is not None:
            out[2][l] = blend_level(out[2][l], f32(t_pitch[l]), w_pitch[l])
    return out[0], out[1], out[2], exact


def impose_durations(exact, t_dur, length, dur, durations_int, total, status, hop_length=256, sampling_rate=22050):
    ''' one row of dx_prosody_impose_durations on K16's results.  Returns (dur fp32, durations_int, total, status). '''
    dur, durations_int = np.asarray(dur, dtype=np.float32).copy(), np.asarray(durations_int, dtype=np.int64).copy()
    if exact == 0:
        return dur, durations_int, int(total), int(status)
    if exact < 0:
        return dur, durations_int, int(total), ST_WEIGHT
    n = int(length)
    durations_int[:] = 0
    durations_int[:n] = [int(t) for t in t_dur[:n]]
    for l in range(n):
        dur[l] = target_seconds(t_dur[l], hop_length, sampling_rate)
    total = int(durations_int.sum())
    return dur, durations_int, total, 0 if total > 0 else ST_EMPTY


# ---- the forced synthesis, stage by stage (oracle/daft_exprt_cpu.py) ----------------------------------------------------------------

def forced_inference(P, hp, inputs, t_dur, t_energy, t_pitch):
    ''' inference with full targets at weight 1 and neutral factors ('multiply' 0: the pitch transform is then the identity), as
        the composition of the CPU oracle's own stages: prosody_encoder -> phoneme_encoder -> prosody_predictor -> impose ->
        gaussian_upsampling -> frame_decoder.  inputs: the 10-tuple of `inference` (CPU tensors); t_dur (B, L) int64 frames,
        t_energy / t_pitch (B, L) fp32, all zero past the input lengths.  The imposed values are the targets themselves, the
        duration in seconds; energy and pitch are zeroed where a symbol has 0 frames (the rule of `inference`).
        Returns ([dur, dur_int, energy, pitch], [mel, output_lengths]). '''
    import torch
    from oracle import daft_exprt_cpu as O
    symbols, _, _, _, input_lengths, energy_refs, pitch_refs, mel_spec_refs, ref_lengths, speaker_ids = inputs
    with torch.no_grad():
        _, enc_film, pp_film, dec_film = O.prosody_encoder(P, hp, energy_refs, pitch_refs, mel_spec_refs, speaker_ids, ref_lengths, False)
        enc = O.phoneme_encoder(P, hp, symbols, enc_film, input_lengths, False)
        dur, energy, pitch = (t.clone() for t in O.prosody_predictor(P, hp, enc, pp_film, input_lengths, False))
        live = O.valid_mask(input_lengths, symbols.shape[1])
        seconds = torch.tensor([[float(target_seconds(f, hp.hop_length, hp.sampling_rate)) for f in row] for row in t_dur.tolist()],
                               dtype=torch.float32)
        dur = torch.where(live, seconds, dur)
        dur_int = torch.where(live, t_dur, torch.zeros_like(t_dur))
        silent = dur_int == 0
        energy = torch.where(live, t_energy, energy).masked_fill(silent, 0.)
        pitch = torch.where(live, t_pitch, pitch).masked_fill(silent, 0.)
        x_up, _ = O.gaussian_upsampling(P, hp, enc, dur, dur_int, energy, pitch, input_lengths)
        output_lengths = dur_int.sum(dim=1)
        mel = O.frame_decoder(P, hp, x_up, dec_film, output_lengths, False)
    return [dur, dur_int, energy, pitch], [mel, output_lengths]
