"""Objective prosody-transfer scores on the GPU (reference: `scripts/evaluation/compare_pitch_curves.py:5-45`).

The reference's only objective measure of prosody transfer is Pearson's correlation between the pitch curve of a generated
utterance and the one of its prosody reference, after dropping the unvoiced frames of both and Fourier-resampling the
generated curve to the reference's length.  `dx_curve_pcc` (csrc/prosody_eval.hip) computes it for a batch of curve pairs,
one workgroup per pair; `prosody_transfer_scores` applies it to a batch of generated waveforms -- pitch tracked and energy
analysed on the device -- against the collated reference curves, which is what `generate.generate_batch_mel_specs(scores=...)`
reports per file.  No CPU fallback: without the HIP library / a GPU these functions raise.

Where this differs from the reference, by design: an empty curve after unvoiced removal (the reference raises ValueError when
it is the generated one) and a zero standard deviation give NaN, for either curve.
"""
import numpy as np
import torch

from daft_exprt import _hip as H


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
    from daft_exprt.extract_features import mel_spectrogram_batch, pitch_batch
    H.require_gpu(wavs, n_samples, pitch_refs, energy_refs, ref_lengths)
    pitch, n_pitch = pitch_batch(wavs, n_samples, hparams)
    _, energy, n_frames = mel_spectrogram_batch(wavs, n_samples, hparams)
    pitch_refs, energy_refs = pitch_refs.float().contiguous(), energy_refs.float().contiguous()
    pitch_pcc, voiced_ref, voiced_gen = curve_pcc_batch(pitch_refs, ref_lengths, pitch, n_pitch, remove_unvoiced=True)
    energy_pcc, frames_ref, frames_gen = curve_pcc_batch(energy_refs, ref_lengths, energy, n_frames, remove_unvoiced=False)
    return dict(zip(SCORE_KEYS, (pitch_pcc, energy_pcc, voiced_ref, voiced_gen, frames_ref, frames_gen)))
