"""Audio I/O of the vocoder fine-tuning data set (reference: `fine_tune.py:92-115`, `extract_features.py:362-384`).

`load_wav(path, sr)` keeps the contract of the reference's `librosa.load(path, sr=sr)`: float32 samples in [-1, 1), averaged
to mono, resampled to `sr` when the file's rate differs.  The file is read with the standard library (RIFF / WAVE, PCM 16-bit
or 32-bit IEEE float); the resampling runs on the device (`dx_resample`, csrc/audio.hip), `resample_batch` is its batched
device entry.  No CPU fallback: resampling without the HIP library / a GPU raises.

The resampler restates what librosa 0.8.1 `resample(res_type='kaiser_best')` hands to resampy 0.2.x: a windowed-sinc
interpolator with NUM_ZEROS zero crossings per wing at 2^PRECISION table points per crossing, ROLLOFF and a Kaiser window of
KAISER_BETA; output length ceil(n * sr_out / sr_in) (resampy's floor, zero-padded by librosa's fix_length).  These constants
and rules are NOT pinned against either library (neither is a dependency of this project, and no recording of their output
is kept in the tests); they are restated from their published source, as the mel filterbank of `extract_features.py` is.
Two details are exact here where the originals use floating point: the input position of output sample t is
floor(t * sr_in / sr_out) with its fraction from the integer remainder (resampy accumulates 1 / ratio), and the output length
uses integer arithmetic (librosa: np.ceil of a float product).
"""
import functools
import math
import struct
from types import SimpleNamespace

import numpy as np
import torch

from daft_exprt import _hip as H

NUM_ZEROS = 64
PRECISION = 9
ROLLOFF = 0.9475937167399596
KAISER_BETA = 14.769656459379492


@functools.lru_cache(maxsize=1)
def filter_table():
    ''' (table (NUM_ZEROS * 2^PRECISION + 1,) float64, 2^PRECISION): the right half of the windowed sinc, one point every
        2^-PRECISION zero crossings '''
    n_bits = 2 ** PRECISION
    n = n_bits * NUM_ZEROS
    sinc = ROLLOFF * np.sinc(ROLLOFF * np.linspace(0, NUM_ZEROS, num=n + 1, endpoint=True))
    taper = np.kaiser(2 * n + 1, KAISER_BETA)[n:]
    return sinc * taper, n_bits


def out_length(n_in, sr_in, sr_out):
    ''' samples librosa returns for n_in samples: ceil(n_in * sr_out / sr_in) '''
    return -(-int(n_in) * int(sr_out) // int(sr_in))


def resample_bank(sr_in, sr_out):
    ''' (bank (taps, P) float64, left): the polyphase bank of sr_in -> sr_out, P = sr_out / gcd.  Phase r serves every output
        t = r mod P; its tap j weighs x[floor(t sr_in / sr_out) - (left - 1) + j].  Built exactly as resampy reads its table:
        wing offsets scale * f and scale * (1 - f) zero crossings (f from the integer remainder), step int(scale * 2^PRECISION)
        table points, linear interpolation, times scale when downsampling. '''
    sr_in, sr_out = int(sr_in), int(sr_out)
    g = math.gcd(sr_in, sr_out)
    P, Q = sr_out // g, sr_in // g
    win, n_bits = filter_table()
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    ratio = float(sr_out) / sr_in
    scale = min(1.0, ratio)
    step = int(scale * n_bits)
    nwin = win.shape[0]
    f = ((np.arange(P, dtype=np.int64) * Q) % P) / P
    frac_l = scale * f
    wings = []
    for frac in (frac_l, scale - frac_l):
        index = frac * n_bits
        offset = index.astype(np.int64)
        wings.append((offset, index - offset, (nwin - offset) // step))
    left, right = int(wings[0][2].max()), int(wings[1][2].max())
    taps = left + right
    cap = int(H.lib().dx_resample_max_weights())
    if P * taps > cap:
        raise ValueError(f'resample {sr_in} -> {sr_out} Hz: the polyphase bank has {P} phases x {taps} taps = {P * taps} weights, '
                         f'more than the {cap} supported')
    bank = np.zeros((taps, P), dtype=np.float64)
    for side, (offset, eta, count) in enumerate(wings):
        for i in range(int(count.max())):
            live = i < count
            pos = np.where(live, offset + i * step, 0)
            w = np.where(live, win[pos] + eta * delta[pos], 0.)
            bank[left - 1 - i if side == 0 else left + i] = w
    if ratio < 1:
        bank *= scale
    return bank, left


def _device_bank(sr_in, sr_out, device):
    def make():
        bank, left = resample_bank(sr_in, sr_out)
        return torch.from_numpy(bank.astype(np.float32)).to(device), left
    return H.device_table('resample', device, int(sr_in), int(sr_out), make=make)


def fft_tables(n_fft, symmetric, device):
    ''' (twiddle (2 n_fft,) fp32: exp(-2 pi i t / n_fft) as (cos, sin) pairs, Hann window (n_fft,) fp32) of the in-LDS FFT on
        `device`: the periodic window of `torch.hann_window` (the STFT of the mel front-end) or, with `symmetric`, `np.hanning`
        (Griffin-Lim).  The table entry points write both; the twiddles do not depend on the window, so those of the first
        call are kept for both kinds. '''
    def make_window():
        twiddle = torch.empty(2 * n_fft, dtype=torch.float32, device=device)
        window = torch.empty(n_fft, dtype=torch.float32, device=device)
        tables = H.lib().dx_gl_tables if symmetric else H.lib().dx_mel_tables
        H.check(tables(H.ptr(twiddle), H.ptr(window), n_fft, H.stream()))
        H.device_table('twiddle', device, n_fft, make=lambda: twiddle)
        return window
    window = H.device_table('window', device, n_fft, bool(symmetric), make=make_window)
    return H.device_table('twiddle', device, n_fft), window


def resample_batch(wavs, n_in, sr_in, sr_out):
    ''' wavs (B, S) fp32 device tensor (right-padded), n_in (B,) int64 device tensor, both rates in Hz.  Returns
        (y (B, ceil(S * sr_out / sr_in)) fp32, n_out (B,) int64 = ceil(n_in * sr_out / sr_in)), both on the device, zeros past
        n_out[b].  Equal rates copy the input (librosa does not resample them). '''
    H.require_gpu(wavs, n_in)
    assert wavs.dtype == torch.float32 and wavs.dim() == 2 and wavs.stride(1) == 1 and n_in.dtype == torch.int64
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in <= 0 or sr_out <= 0:
        raise ValueError(f'resample: rates must be positive, got {sr_in} -> {sr_out} Hz')
    B, S = wavs.shape
    S_out = out_length(S, sr_in, sr_out)
    y = torch.empty((B, S_out), dtype=torch.float32, device=wavs.device)
    n_out = torch.empty((B,), dtype=torch.int64, device=wavs.device)
    bank, taps, left = None, 0, 0
    if sr_in != sr_out:
        bank, left = _device_bank(sr_in, sr_out, wavs.device)
        taps = bank.shape[0]
    H.check(H.lib().dx_resample(H.ptr(wavs), wavs.stride(0), H.ptr(n_in), H.ptr(bank), H.ptr(y), S_out, H.ptr(n_out), B, S,
                                S_out, sr_in, sr_out, taps, left, H.stream()))
    return y, n_out


def ft_pack(mel, lengths, wavs, crop, mel_total, wav_total):
    ''' `dx_ft_pack`: mel (B, n_mel, T) fp32 and lengths (B,) int64, wavs (B, S) fp32 and crop (B, 2) int64 (begin, length), all
        on the device; mel_total = n_mel * sum of min(lengths, T), wav_total = sum of crop lengths (host values).  Returns one
        uint8 device buffer: the cropped mels back to back (fp32), then the cropped int16 waveforms back to back. '''
    H.require_gpu(mel, lengths, wavs, crop)
    assert mel.dtype == torch.float32 and mel.stride(2) == 1 and wavs.dtype == torch.float32 and wavs.stride(1) == 1
    assert lengths.dtype == torch.int64 and crop.dtype == torch.int64 and crop.is_contiguous()
    B, n_mel, T = mel.shape
    mel_bytes = 4 * int(mel_total)
    buf = torch.empty((mel_bytes + 2 * int(wav_total) + 4,), dtype=torch.uint8, device=mel.device)
    H.check(H.lib().dx_ft_pack(H.ptr(mel), mel.stride(0), mel.stride(1), H.ptr(lengths), B, n_mel, T, H.ptr(wavs), wavs.stride(0),
                               H.ptr(crop), wavs.shape[1], H.ptr(buf), buf.data_ptr() + mel_bytes, H.stream()))
    return buf[:mel_bytes + 2 * int(wav_total)]


def crop_range(sent_begin, sent_end, fs, n_samples):
    ''' (begin, length) of `wav[int(sent_begin * fs): int(sent_end * fs)]` for a wav of n_samples (`fine_tune.py:100`,
        `extract_features.py:426`), with Python's slice rules '''
    r = range(int(n_samples))[int(sent_begin * fs): int(sent_end * fs)]
    return (r.start, len(r)) if len(r) else (0, 0)


def resampled_length(utt, fs):
    ''' samples `utt` (`.samples`, `.rate`) holds at fs; a rate of fs keeps the count '''
    return out_length(len(utt.samples), utt.rate, fs)


def device_waves(utts, fs, device):
    ''' utts: objects with `.samples` (mono float32 NumPy) and `.rate`.  Returns the (B, S) fp32 device waveforms at fs, zeros
        past each length, and their lengths (host ints): one H2D copy per source rate and, for every one other than fs, one
        resample launch '''
    n_total = [resampled_length(u, fs) for u in utts]
    wavs = torch.zeros((len(utts), max(max(n_total), 1)), dtype=torch.float32, device=device)
    for rate in sorted(set(u.rate for u in utts)):
        rows = [b for b, u in enumerate(utts) if u.rate == rate]
        n_in = [len(utts[b].samples) for b in rows]
        host = torch.zeros((len(rows), max(max(n_in), 1)), dtype=torch.float32).pin_memory()
        for i, b in enumerate(rows):
            host[i, :n_in[i]] = torch.from_numpy(utts[b].samples)
        x = host.to(device, non_blocking=True)
        if rate != fs:
            n_dev = torch.tensor(n_in, dtype=torch.int64).pin_memory().to(device, non_blocking=True)
            x, _ = resample_batch(x, n_dev, rate, fs)
        idx = torch.tensor(rows, dtype=torch.int64).pin_memory().to(device, non_blocking=True)
        wavs[:, :x.shape[1]].index_copy_(0, idx, x)
    return wavs, n_total


# ---- WAV files ------------------------------------------------------------------------------------------------------------

_KSDATAFORMAT_TAIL = b'\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71'    # WAVE_FORMAT_EXTENSIBLE sub-format GUID tail


def read_wav(path):
    ''' (samples (n, channels) as stored -- int16 or float32 --, sampling rate) of a RIFF / WAVE file holding PCM 16-bit or
        32-bit IEEE float samples (plain or WAVE_FORMAT_EXTENSIBLE); any other format raises ValueError '''
    with open(path, 'rb') as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b'RIFF' or data[8:12] != b'WAVE':
        raise ValueError(f'{path}: not a RIFF / WAVE file')
    pos, fmt, samples = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack('<I', data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b'fmt ':
            if size < 16:
                raise ValueError(f'{path}: truncated fmt chunk')
            tag, channels, rate, _, block, bits = struct.unpack('<HHIIHH', body[:16])
            if tag == 0xFFFE and size >= 40 and body[26:40] == _KSDATAFORMAT_TAIL:
                tag = struct.unpack('<H', body[24:26])[0]
            fmt = (tag, channels, rate, block, bits)
        elif cid == b'data':
            samples = body
        pos += 8 + size + (size & 1)
    if fmt is None or samples is None:
        raise ValueError(f'{path}: no {"fmt" if fmt is None else "data"} chunk')
    tag, channels, rate, block, bits = fmt
    if tag == 1 and bits == 16:
        dtype = '<i2'
    elif tag == 3 and bits == 32:
        dtype = '<f4'
    else:
        name = {1: 'PCM', 3: 'IEEE float', 6: 'A-law', 7: 'mu-law', 2: 'ADPCM'}.get(tag, f'format tag {tag:#x}')
        raise ValueError(f'{path}: {name} {bits}-bit samples are not supported (PCM 16-bit or IEEE float 32-bit)')
    if channels < 1:
        raise ValueError(f'{path}: {channels} channels')
    n = len(samples) // (channels * bits // 8)
    x = np.frombuffer(samples[:n * channels * bits // 8], dtype=dtype).reshape(n, channels)
    return x.astype(np.int16 if tag == 1 else np.float32), int(rate)


def to_float_mono(x):
    ''' (n, channels) int16 / float32 -> (n,) float32: int16 / 32768, channels averaged (librosa.to_mono) '''
    y = x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x.astype(np.float32)
    return y[:, 0].copy() if y.shape[1] == 1 else np.mean(y, axis=1, dtype=np.float32)


def load_wav(path, sr=22050, device=None):
    ''' `librosa.load(path, sr=sr)`: (float32 samples, sr); sr=None keeps the file's rate.  A file of another rate is
        resampled on the device (`device`, default cuda:0). '''
    y, rate = read_wav(path)
    y = to_float_mono(y)
    if sr is None or int(sr) == rate:
        return y, rate
    wavs, n = device_waves([SimpleNamespace(samples=y, rate=rate)], int(sr), H.device(device))
    return wavs[0, :n[0]].cpu().numpy(), int(sr)


def rescale_wav_to_float32(x):
    ''' `extract_features.py:362-384`: int16 / int32 / uint8 / float samples -> float32 in [-1, 1] (amplitudes above 1 are
        let through, as in the reference) '''
    if x.dtype == 'int16':
        y = x / 32768.0
    elif x.dtype == 'int32':
        y = x / 2147483648.0
    elif x.dtype == 'uint8':
        y = ((x / 255.0) - 0.5) * 2
    elif x.dtype == 'float32' or x.dtype == 'float64':
        y = x
    else:
        raise TypeError(f'could not normalize wav, unsupported sample type {x.dtype}')
    return y.astype('float32')


def _wav_header(tag, sampling_rate, sample_bytes, n_samples, fmt_tail=b'', chunks=b''):
    ''' RIFF / WAVE header of n_samples mono samples of sample_bytes each: the `fmt ` chunk (format `tag`, closed by
        `fmt_tail`), `chunks` as they stand, and the header of the `data` chunk, whose samples the caller appends '''
    rate, nbytes = int(sampling_rate), sample_bytes * int(n_samples)
    fmt = struct.pack('<HHIIHH', tag, 1, rate, rate * sample_bytes, sample_bytes, 8 * sample_bytes) + fmt_tail
    body = b'WAVE' + b'fmt ' + struct.pack('<I', len(fmt)) + fmt + chunks + b'data' + struct.pack('<I', nbytes)
    return b'RIFF' + struct.pack('<I', len(body) + nbytes) + body


def wav_int16_header(sampling_rate, n_samples):
    ''' the 44-byte header `scipy.io.wavfile.write` puts in front of n_samples int16 mono samples '''
    return _wav_header(1, sampling_rate, 2, n_samples)


def write_wav_int16(path, sampling_rate, data):
    ''' int16 mono WAV, byte for byte what `scipy.io.wavfile.write(path, sampling_rate, data)` writes for int16 data '''
    data = np.ascontiguousarray(np.asarray(data).reshape(-1))
    assert data.dtype == np.int16, data.dtype
    with open(path, 'wb') as f:
        f.write(wav_int16_header(sampling_rate, data.size))
        f.write(data.astype('<i2', copy=False).tobytes())


def write_wav(path, sampling_rate, data):
    ''' mono 64-bit IEEE-float WAV -- what `scipy.io.wavfile.write` makes of the reference's float64 waveform
        (generate.py:137): RIFF / WAVE, `fmt ` (format 3, 18 bytes: cbSize = 0), `fact` (the sample count), `data` '''
    data = np.ascontiguousarray(np.asarray(data, dtype='<f8').reshape(-1))
    fact = b'fact' + struct.pack('<II', 4, data.size)
    with open(path, 'wb') as f:
        f.write(_wav_header(3, sampling_rate, 8, data.size, fmt_tail=struct.pack('<H', 0), chunks=fact))
        f.write(data.tobytes())
