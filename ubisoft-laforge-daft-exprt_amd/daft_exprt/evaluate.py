"""Objective prosody-transfer scores on the GPU (reference: `scripts/evaluation/compare_pitch_curves.py:5-45`).

The reference's only objective measure of prosody transfer is Pearson's correlation between the pitch curve of a generated
utterance and the one of its prosody reference, after dropping the unvoiced frames of both and Fourier-resampling the
generated curve to the reference's length.  `dx_curve_pcc` (csrc/prosody_eval.hip) computes it for a batch of curve pairs,
one workgroup per pair; `prosody_transfer_scores` applies it to a batch of generated waveforms -- pitch tracked and energy
analysed on the device -- against the collated reference curves, which is what `generate.generate_batch_mel_specs(scores=...)`
reports per file.  No CPU fallback: without the HIP library / a GPU these functions raise.

Further down, an addition the reference has no counterpart of: copy-synthesis scores.  `copy_synthesis_scores` synthesises a
data-loader batch free-running with every utterance's own recording as prosody reference and compares the result with that
recording along a dynamic-time-warping path of the two mel cepstra (csrc/dtw_eval.hip): mel-cepstral distortion, F0 RMSE in
cents and voicing error, at the level of the decoder's mel and of the vocoded (or Griffin-Lim) audio; `scripts/evaluate.py`
reports them for a file list.

Where this differs from the reference, by design: an empty curve after unvoiced removal (the reference raises ValueError when
it is the generated one) and a zero standard deviation give NaN, for either curve.
"""
import numpy as np
import torch

from daft_exprt import _hip as H
from daft_exprt import config, griffin_lim
from daft_exprt.extract_features import mel_spectrogram_batch, pitch_batch
from daft_exprt.recordings import copy_inference, max_dtw_length, unwrap


def max_curve_length():
    ''' longest curve (frames before unvoiced removal) `curve_pcc_batch` takes '''
    return int(H.lib().dx_curve_pcc_max_len())


def curve_pcc_batch(ref, n_ref, dut, n_dut, remove_unvoiced=True, return_resampled=False):
    ''' ref (B, T_ref) / dut (B, T_dut) fp32 device tensors (right-padded), n_ref / n_dut (B,) int64 device tensors.
        Returns (pcc (B,) fp32, kept_ref (B,) int32, kept_dut (B,) int32[, resampled (B, T_ref) fp32]) on the device: per row
        the correlation of ref[:n_ref] with dut[:n_dut] resampled to its length, both without their values <= 0 when
        `remove_unvoiced`; the lengths left; the resampled curve in [0, kept_ref) (zeros behind it).  NaN where a curve is
        left empty or has no variation.  Nothing at or past n_ref / n_dut is read. '''
    H.require_gpu(ref, n_ref, dut, n_dut)
    assert ref.dtype == torch.float32 and dut.dtype == torch.float32 and n_ref.dtype == torch.int64 and n_dut.dtype == torch.int64
    assert ref.dim() == 2 and dut.dim() == 2 and ref.stride(1) == 1 and dut.stride(1) == 1
    B, T_ref = ref.shape
    assert dut.shape[0] == B and n_ref.shape == (B,) and n_dut.shape == (B,)
    dev = ref.device
    pcc = torch.empty((B,), dtype=torch.float32, device=dev)
    kept_ref = torch.empty((B,), dtype=torch.int32, device=dev)
    kept_dut = torch.empty((B,), dtype=torch.int32, device=dev)
    resampled = torch.zeros((B, T_ref), dtype=torch.float32, device=dev) if return_resampled else None
    H.check(H.lib().dx_curve_pcc(H.ptr(ref), ref.stride(0), H.ptr(n_ref.contiguous()), H.ptr(dut), dut.stride(0),
                                 H.ptr(n_dut.contiguous()), H.ptr(pcc), H.ptr(kept_ref), H.ptr(kept_dut), H.ptr(resampled),
                                 T_ref if return_resampled else 0, B, T_ref, dut.shape[1], int(bool(remove_unvoiced)), H.stream()))
    return (pcc, kept_ref, kept_dut, resampled) if return_resampled else (pcc, kept_ref, kept_dut)


def pcc_on_2_pitch_curve(ref, dut, remove_unvoiced=True, device=None):
    ''' reference signature (`compare_pitch_curves.py:24`): two curves of arbitrary lengths (unvoiced where <= 0) -> float '''
    dev = H.device(device)
    r = torch.as_tensor(np.asarray(ref, dtype=np.float32)).reshape(1, -1)
    d = torch.as_tensor(np.asarray(dut, dtype=np.float32)).reshape(1, -1)
    n_r, n_d = r.shape[1], d.shape[1]
    if n_r == 0 or n_d == 0:
        return float('nan')
    pcc, _, _ = curve_pcc_batch(r.to(dev), torch.tensor([n_r], dtype=torch.int64, device=dev), d.to(dev),
                                torch.tensor([n_d], dtype=torch.int64, device=dev), remove_unvoiced)
    return float(pcc[0])


SCORE_KEYS = ('pitch_pcc', 'energy_pcc', 'voiced_ref', 'voiced_gen', 'frames_ref', 'frames_gen')


def prosody_transfer_scores(wavs, n_samples, pitch_refs, energy_refs, ref_lengths, hparams):
    ''' wavs (B, S) fp32 / n_samples (B,) int64: generated waveforms on the device (`griffin_lim.griffin_lim_batch`'s output);
        pitch_refs, energy_refs (B, T) fp32 and ref_lengths (B,) int64: the collated reference curves on the device
        (`generate.collate_tensors` columns 6, 5 and 8).  The waveforms are pitch-tracked and analysed (`pitch_batch`,
        `mel_spectrogram_batch`), then two `curve_pcc_batch` calls: pitch without the unvoiced frames, energy over all frames.
        Returns {key: (B,) device tensor} for SCORE_KEYS: the two correlations (fp32, NaN where undefined), the voiced frames
        of reference and generated pitch, the frames of reference and generated utterance. '''
    H.require_gpu(wavs, n_samples, pitch_refs, energy_refs, ref_lengths)
    pitch, n_pitch = pitch_batch(wavs, n_samples, hparams)
    _, energy, n_frames = mel_spectrogram_batch(wavs, n_samples, hparams)
    pitch_refs, energy_refs = pitch_refs.float().contiguous(), energy_refs.float().contiguous()
    pitch_pcc, voiced_ref, voiced_gen = curve_pcc_batch(pitch_refs, ref_lengths, pitch, n_pitch, remove_unvoiced=True)
    energy_pcc, frames_ref, frames_gen = curve_pcc_batch(energy_refs, ref_lengths, energy, n_frames, remove_unvoiced=False)
    return dict(zip(SCORE_KEYS, (pitch_pcc, energy_pcc, voiced_ref, voiced_gen, frames_ref, frames_gen)))


# ---- copy synthesis: how close the free-running path gets to a recording of the same text ----------------------------------------
# Mel-cepstral distortion, F0 RMSE and voicing error along the path of a dynamic time warping of the two mel cepstra
# (csrc/dtw_eval.hip: `dx_mel_cepstrum`, `dx_dtw_align`, `dx_dtw_path_scores`).  The mel of this project is a natural log, so the
# cepstra are natural-log cepstra and MCD = (10 sqrt(2) / ln 10) x the mean Euclidean distance over coefficients 1..K.

DTW_KEYS = ('mcd_db', 'f0_rmse_cents', 'vuv_error', 'voiced_pairs', 'path_len', 'frames_ref', 'frames_gen')
COPY_LEVELS = ('mel', 'audio')
PER_LEVELS = ('recording', 'mel', 'audio')      # scores['per'] of `copy_synthesis_scores(recognizer=...)`
SPEAKER_LEVELS = PER_LEVELS                      # scores['speaker'] of `copy_synthesis_scores(speaker_encoder=...)`
DTW_WORKSPACE_BYTES = 256 << 20         # default cap of the direction workspace: 256 pairs of 1000 x 1000 frames take 64 MB
_DTW_WORKSPACE = {}                     # device -> grow-only byte tensor, kept across calls


def _dct_table(n_mel, n_coeffs, device):
    def make():
        k = np.arange(1, n_coeffs + 1, dtype=np.float64)[:, None]
        m = np.arange(n_mel, dtype=np.float64)[None, :]
        table = np.sqrt(2.0 / n_mel) * np.cos(np.pi * (m + 0.5) * k / n_mel)       # rows 1..K of the orthonormal DCT-II, in double
        return torch.from_numpy(table.astype(np.float32)).to(device)                # rounded once
    return H.device_table('mel_cepstrum_dct', device, n_mel, n_coeffs, make=make)


def mel_cepstrum_batch(mel, lengths, n_coeffs=13):
    ''' mel (B, n_mel, T) fp32 device tensor (natural-log mel, right-padded), lengths (B,) int64 -> cepstra (B, T, K) fp32,
        time-major: coefficients 1..K of the orthonormal DCT-II over the mel axis (c0 dropped), zeros at and past lengths[b].
        Nothing at or past lengths[b] is read. '''
    H.require_gpu(mel, lengths)
    assert mel.dtype == torch.float32 and lengths.dtype == torch.int64 and mel.dim() == 3 and mel.stride(2) == 1
    B, n_mel, T = mel.shape
    assert lengths.shape == (B,)
    if not 1 <= n_coeffs < n_mel:
        raise ValueError(f'n_coeffs = {n_coeffs}: the cepstrum keeps coefficients 1..K with 1 <= K < n_mel = {n_mel}')
    cep = torch.empty((B, T, n_coeffs), dtype=torch.float32, device=mel.device)
    H.check(H.lib().dx_mel_cepstrum(H.ptr(mel), mel.stride(0), mel.stride(1), H.ptr(lengths.contiguous()),
                                    H.ptr(_dct_table(n_mel, n_coeffs, mel.device)), H.ptr(cep), B, n_mel, T, n_coeffs, H.stream()))
    return cep


def dtw_align_batch(cep_ref, n_ref, cep_gen, n_gen, max_workspace_bytes=DTW_WORKSPACE_BYTES):
    ''' cep_ref (B, T_ref, K) / cep_gen (B, T_gen, K) fp32 device tensors, n_ref / n_gen (B,) int64.  Returns
        (total (B,) fp32, path (B, T_ref + T_gen - 1, 2) int32, path_len (B,) int32) on the device: per pair the accumulated
        cost and the cells of the unconstrained DTW of cep_ref[b, :n_ref[b]] against cep_gen[b, :n_gen[b]] (Euclidean local cost;
        among equal predecessors the diagonal, then (i-1, j), then (i, j-1)); -1 behind path_len[b]; path_len 0 and total NaN
        where a sequence is empty.  The 2-bit direction codes need T_ref * ceil(T_gen / 4) bytes per pair -- the batch's own padded
        extents, not the limit --: the batch is walked in sub-batches that keep them under `max_workspace_bytes` (one pair at least),
        in one grow-only workspace per device that is kept across calls (DX_POISON=1 fills it with 0xFF first). '''
    H.require_gpu(cep_ref, n_ref, cep_gen, n_gen)
    assert cep_ref.dtype == torch.float32 and cep_gen.dtype == torch.float32 and n_ref.dtype == torch.int64 and n_gen.dtype == torch.int64
    assert cep_ref.dim() == 3 and cep_gen.dim() == 3 and cep_ref.is_contiguous() and cep_gen.is_contiguous()
    B, T_ref, K = cep_ref.shape
    T_gen = cep_gen.shape[1]
    assert cep_gen.shape == (B, T_gen, K) and n_ref.shape == (B,) and n_gen.shape == (B,)
    dev = cep_ref.device
    n_ref, n_gen = n_ref.contiguous(), n_gen.contiguous()
    total = torch.empty((B,), dtype=torch.float32, device=dev)
    path = torch.empty((B, T_ref + T_gen - 1, 2), dtype=torch.int32, device=dev)
    path_len = torch.empty((B,), dtype=torch.int32, device=dev)
    per_pair = T_ref * ((T_gen + 3) // 4)
    step = max(1, min(B, int(max_workspace_bytes) // max(per_pair, 1)))
    ws = _DTW_WORKSPACE.get(dev)
    if ws is None or ws.numel() < step * per_pair:
        ws = _DTW_WORKSPACE[dev] = torch.empty((step * per_pair,), dtype=torch.uint8, device=dev)
    if config.POISON:
        ws.fill_(0xFF)                  # four times the code that stands for no predecessor: every byte read must have been written
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        H.check(H.lib().dx_dtw_align(H.ptr(cep_ref[b0:b1]), H.ptr(n_ref[b0:b1]), H.ptr(cep_gen[b0:b1]), H.ptr(n_gen[b0:b1]),
                                     H.ptr(total[b0:b1]), H.ptr(path[b0:b1]), H.ptr(path_len[b0:b1]), H.ptr(ws), per_pair, b1 - b0,
                                     T_ref, T_gen, K, H.stream()))
    return total, path, path_len


def dtw_path_scores_batch(cep_ref, n_ref, cep_gen, n_gen, path, path_len, pitch_ref=None, pitch_gen=None):
    ''' the reduction along given paths (`dx_dtw_path_scores`): (mcd_db, f0_rmse_cents, vuv_error (B,) fp32, voiced_pairs, path_len
        (B,) int32).  pitch_ref (B, >= T_ref) / pitch_gen (B, >= T_gen): raw log-Hz curves, <= 0 where unvoiced, or both None. '''
    H.require_gpu(cep_ref, n_ref, cep_gen, n_gen, path, path_len, pitch_ref, pitch_gen)
    B, T_ref, K = cep_ref.shape
    T_gen = cep_gen.shape[1]
    assert cep_ref.is_contiguous() and cep_gen.is_contiguous() and path.is_contiguous() and path.dtype == torch.int32
    assert path.shape == (B, T_ref + T_gen - 1, 2) and path_len.dtype == torch.int32 and (pitch_ref is None) == (pitch_gen is None)
    ld_ref = ld_gen = 0
    if pitch_ref is not None:
        pitch_ref, pitch_gen = pitch_ref.float(), pitch_gen.float()
        assert pitch_ref.stride(1) == 1 and pitch_gen.stride(1) == 1 and pitch_ref.shape[1] >= T_ref and pitch_gen.shape[1] >= T_gen
        ld_ref, ld_gen = pitch_ref.stride(0), pitch_gen.stride(0)
    dev = cep_ref.device
    mcd, f0, vuv = (torch.empty((B,), dtype=torch.float32, device=dev) for _ in range(3))
    voiced, used = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(2))
    H.check(H.lib().dx_dtw_path_scores(H.ptr(cep_ref), H.ptr(n_ref.contiguous()), H.ptr(cep_gen), H.ptr(n_gen.contiguous()), H.ptr(path),
                                       H.ptr(path_len.contiguous()), H.ptr(pitch_ref), ld_ref, H.ptr(pitch_gen), ld_gen, H.ptr(mcd),
                                       H.ptr(f0), H.ptr(vuv), H.ptr(voiced), H.ptr(used), B, T_ref, T_gen, K, H.stream()))
    return mcd, f0, vuv, voiced, used


def dtw_scores_batch(mel_ref, n_ref, mel_gen, n_gen, pitch_ref=None, pitch_gen=None, n_coeffs=13):
    ''' mel_ref (B, n_mel, T_ref) / mel_gen (B, n_mel, T_gen) fp32 device tensors with n_ref / n_gen (B,) int64 frames, and
        optionally the raw log-Hz pitch curves pitch_ref (B, T_ref) / pitch_gen (B, T_gen) (<= 0 where unvoiced).  Cepstra, DTW
        and the reduction along the path, all on the device.  Returns {key: (B,) device tensor} for DTW_KEYS: MCD in dB, F0 RMSE
        in cents over the path pairs voiced on both sides, the share of path pairs voiced on one side only (both NaN without
        pitch curves), the doubly voiced pairs, the path length and the two frame counts.  A pair with an empty side scores NaN. '''
    H.require_gpu(mel_ref, n_ref, mel_gen, n_gen, pitch_ref, pitch_gen)
    cep_ref = mel_cepstrum_batch(mel_ref, n_ref, n_coeffs)
    cep_gen = mel_cepstrum_batch(mel_gen, n_gen, n_coeffs)
    _, path, path_len = dtw_align_batch(cep_ref, n_ref, cep_gen, n_gen)
    mcd, f0, vuv, voiced, used = dtw_path_scores_batch(cep_ref, n_ref, cep_gen, n_gen, path, path_len, pitch_ref, pitch_gen)
    frames_ref = n_ref.clamp(0, mel_ref.shape[2]).to(torch.int32)
    frames_gen = n_gen.clamp(0, mel_gen.shape[2]).to(torch.int32)
    return dict(zip(DTW_KEYS, (mcd, f0, vuv, voiced, used, frames_ref, frames_gen)))


def mcd_dtw(mel_a, mel_b, n_coeffs=13, device=None):
    ''' two natural-log mel-spectrograms (n_mel, T_a), (n_mel, T_b) as NumPy arrays -> their DTW-aligned MCD in dB, a float '''
    dev = H.device(device)
    a = torch.as_tensor(np.asarray(mel_a, dtype=np.float32))
    b = torch.as_tensor(np.asarray(mel_b, dtype=np.float32))
    assert a.dim() == 2 and b.dim() == 2 and a.shape[0] == b.shape[0]
    if a.shape[1] == 0 or b.shape[1] == 0:
        return float('nan')
    n_a = torch.tensor([a.shape[1]], dtype=torch.int64, device=dev)
    n_b = torch.tensor([b.shape[1]], dtype=torch.int64, device=dev)
    return float(dtw_scores_batch(a[None].contiguous().to(dev), n_a, b[None].contiguous().to(dev), n_b, n_coeffs=n_coeffs)['mcd_db'][0])


def copy_synthesis(model, batch, hparams, vocoder=None):
    ''' the free-running synthesis of one collated data-loader batch with every utterance's own recording as prosody reference
        (frames_energy, frames_pitch, mel_specs, output_lengths), its own speaker id, duration and energy factors 1 and pitch
        transform 'add' with factor 0.  Returns (inputs of `parse_batch`, mel (B, n_mel, T) fp32, n_frames (B,) int64,
        wavs (B, S) fp32, n_samples (B,) int64): the decoder's mel and the waveform `vocoder` -- `griffin_lim_batch` when None --
        makes of it. '''
    dev = next(model.parameters()).device
    inputs, _, _ = unwrap(model).parse_batch(dev, batch)
    # symbols, input_lengths, frames_energy, frames_pitch, mel_specs, output_lengths, speaker_ids (the collate has sorted the batch)
    _, (mel, n_frames), _, _ = copy_inference(model, *(inputs[k] for k in (0, 5, 6, 7, 8, 9, 10)), hparams)
    with torch.no_grad():
        mel, n_frames = mel.float().contiguous(), n_frames.long()
        if vocoder is not None:
            vocoder.check_hparams(hparams)
            wavs, n_samples = vocoder(mel, n_frames)
        else:
            wavs, n_samples = griffin_lim.griffin_lim_batch(mel, n_frames, hparams)
    return inputs, mel, n_frames, wavs, n_samples


def copy_synthesis_scores(model, batch, hparams, vocoder=None, n_coeffs=13, recognizer=None, fold=None, speaker_encoder=None):
    ''' one collated data-loader batch (the 13-tuple `DaftExprtDataCollate` returns, `parse_batch`'s input) -> how close the
        free-running synthesis of each utterance (`copy_synthesis`) gets to its own recording.  Returns {'mel': scores,
        'audio': scores}, each {key: (B,) device tensor} for DTW_KEYS, rows in the batch's order:
          mel    the decoder's mel against the recorded mel: MCD and the frame counts (no audio, no pitch: those keys are NaN / 0)
          audio  the waveform, analysed again with `mel_spectrogram_batch` and `pitch_batch`, against the recorded mel and the raw
                 frames_pitch: every key.
        An utterance whose synthesis has 0 frames scores NaN at both levels; it is not dropped.
        `recognizer` (a `recognizer.Recognizer`; with None nothing is launched and nothing returned that was not before) adds
        scores['per']: the phone error rates of `recognizer.phone_error_rates` (its keys, `fold` passed on) against the batch's own
        symbols at the levels PER_LEVELS: `recording` -- the recorded mel, the recogniser's own floor on that utterance --, `mel`
        -- the decoder's mel -- and `audio` -- the re-analysed waveform the DTW scores use.
        `speaker_encoder` (a `speaker.SpeakerEncoder` with centroids; with None nothing is launched and nothing returned that was
        not before) adds scores['speaker']: `speaker.speaker_scores` (cos_target, margin, identified, accepted) against the batch's
        own speaker ids at the same three levels, SPEAKER_LEVELS -- read them together: the recording's row is the encoder's own
        floor on that utterance. '''
    inputs, mel, n_frames, wavs, n_samples = copy_synthesis(model, batch, hparams, vocoder)
    frames_pitch, mel_specs, output_lengths = inputs[7], inputs[8], inputs[9]
    longest = max(mel_specs.shape[2], mel.shape[2])
    if longest > max_dtw_length():
        raise ValueError(f'an utterance of {longest} frames: the DTW takes {max_dtw_length()} at most')
    with torch.no_grad():
        scores = {'mel': dtw_scores_batch(mel_specs, output_lengths, mel, n_frames, n_coeffs=n_coeffs)}
        # the front-end's reflect padding needs more than half a window of samples: shorter rows (an empty synthesis) are not
        # analysed and keep 0 frames
        B, dev = wavs.shape[0], wavs.device
        rows = torch.nonzero((n_frames > 0) & (n_samples > int(hparams.filter_length) // 2)).flatten()
        mel_audio = torch.zeros((B, mel_specs.shape[1], 1), dtype=torch.float32, device=dev)
        pitch = torch.zeros((B, 1), dtype=torch.float32, device=dev)
        n_audio = torch.zeros((B,), dtype=torch.int64, device=dev)
        if rows.numel():
            sub_wavs, sub_n = wavs[rows].contiguous(), n_samples[rows].contiguous()
            sub_pitch, sub_n_pitch = pitch_batch(sub_wavs, sub_n, hparams)
            sub_mel, _, sub_n_mel = mel_spectrogram_batch(sub_wavs, sub_n, hparams)
            T = sub_mel.shape[2]
            mel_audio = torch.zeros((B, sub_mel.shape[1], T), dtype=torch.float32, device=dev)
            pitch = torch.zeros((B, max(T, sub_pitch.shape[1])), dtype=torch.float32, device=dev)
            mel_audio[rows], pitch[rows, :sub_pitch.shape[1]] = sub_mel.float(), sub_pitch.float()
            n_audio[rows] = torch.minimum(sub_n_mel.long(), sub_n_pitch.long())
        scores['audio'] = dtw_scores_batch(mel_specs, output_lengths, mel_audio, n_audio, frames_pitch, pitch, n_coeffs=n_coeffs)
        if recognizer is not None:
            from daft_exprt.recognizer import phone_error_rates
            symbols, input_lengths = inputs[0], inputs[5]
            scores['per'] = {level: phone_error_rates(recognizer, m, n, symbols, input_lengths, fold)
                             for level, m, n in zip(PER_LEVELS, (mel_specs, mel, mel_audio), (output_lengths, n_frames, n_audio))}
        if speaker_encoder is not None:
            from daft_exprt.speaker import speaker_scores
            scores['speaker'] = {level: speaker_scores(speaker_encoder, m, n, batch[10])
                                 for level, m, n in zip(SPEAKER_LEVELS, (mel_specs, mel, mel_audio), (output_lengths, n_frames, n_audio))}
    return scores
