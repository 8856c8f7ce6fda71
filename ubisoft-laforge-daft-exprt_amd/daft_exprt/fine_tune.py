"""Data set for vocoder fine-tuning (reference: `src/daft_exprt/fine_tune.py`).

`fine_tuning(hparams)` runs the trained model teacher-forced over the training set and writes, for every utterance of at
least one second, `<file>.npy` (the float32 (n_mel, T) mel prediction) and `<file>.wav` (int16 ground-truth audio at
`hparams.sampling_rate`, cropped to the span of its markers) under
`os.path.dirname(hparams.training_files)/fine_tuning_dataset/<speaker>/` -- the reference's on-disk result.
`launch_fine_tuning` and the CLI flags `--data_set_dir --config_file --log_file` are the reference's.

Per batch the device work is the eval forward, one `dx_resample` launch per source rate other than `sampling_rate`
(the reference's `librosa.load(..., sr=hparams.sampling_rate)`), one `dx_ft_pack` (crop + int16) and one device-to-host
copy.  The batch's wav files are read on a host thread while the forward runs, and the files are written on another thread
(`write_behind.WriteBehind`), so the next batch's forward never waits for file output.

Differences from the reference, by design:
  * the target mel the reference computes only to compare its shape with the prediction's (`fine_tune.py:101-104`) is not
    computed: its frame count follows from the cropped length (`extract_features.nb_frames`).  A mismatch raises
    ValueError naming the file (the reference asserts);
  * a feature directory that matches no speaker or more than one raises ValueError (the reference asserts).
"""
import argparse
import json
import logging
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from daft_exprt.audio import crop_range, device_waves, ft_pack, read_wav, to_float_mono, write_wav_int16
from daft_exprt.data_loader import prepare_data_loaders
from daft_exprt.extract_features import marker_lines_span, nb_frames
from daft_exprt.hparams import HyperParams
from daft_exprt.model import DaftExprt
from daft_exprt.write_behind import WriteBehind

_logger = logging.getLogger(__name__)


def speaker_of(feature_dir, feature_file, speakers):
    ''' the one speaker whose name ends `feature_dir` (`fine_tune.py:87-89`) '''
    names = [speaker for speaker in speakers if feature_dir.endswith(speaker)]
    if len(names) != 1:
        raise ValueError(f'{feature_dir} -- {feature_file}: {len(names)} speakers match ({names}), expected exactly one')
    return names[0]


def markers_span(markers_file):
    ''' (sent_begin, sent_end) in seconds: begin of the first row, end of the last (`fine_tune.py:96-99`) '''
    with open(markers_file, 'r', encoding='utf-8') as f:
        return marker_lines_span(f.readlines())


class _Utterance(object):
    def __init__(self, feature_dir, feature_file, speaker, samples, rate, span):
        self.feature_dir, self.feature_file, self.speaker = feature_dir, feature_file, speaker
        self.samples, self.rate, self.span = samples, rate, span


def _read_batch(hparams, feature_dirs, feature_files):
    ''' host side of one batch: speaker, mono float32 samples at the file's rate, marker span '''
    out = []
    for feature_dir, feature_file in zip(feature_dirs, feature_files):
        speaker = speaker_of(feature_dir, feature_file, hparams.speakers)
        root = os.path.join(hparams.data_set_dir, speaker)
        x, rate = read_wav(os.path.join(root, 'wavs', f'{feature_file}.wav'))
        span = markers_span(os.path.join(root, 'align', f'{feature_file}.markers'))
        out.append(_Utterance(feature_dir, feature_file, speaker, to_float_mono(x), rate, span))
    return out


class _PackedFiles(object):
    ''' `write` of the pass's `WriteBehind`: the .npy and .wav of every utterance of one packed batch; counts `written` / `skipped` '''
    def __init__(self, hparams, ft_data_set):
        self.fs, self.n_mel, self.root = int(hparams.sampling_rate), int(hparams.n_mel_channels), ft_data_set
        self.written, self.skipped = 0, 0

    def __call__(self, raw, utts, crops, lengths):
        mel_off, wav_off = 0, 4 * self.n_mel * sum(lengths)
        for u, (_, n), T in zip(utts, crops, lengths):
            mel = raw[mel_off: mel_off + 4 * self.n_mel * T].view(np.float32).reshape(self.n_mel, T)
            wav = raw[wav_off: wav_off + 2 * n].view(np.int16)
            mel_off, wav_off = mel_off + 4 * self.n_mel * T, wav_off + 2 * n
            if n < self.fs:
                _logger.warning(f'{u.feature_dir} -- {u.feature_file} -- Ignoring because audio is < 1s')
                self.skipped += 1
                continue
            mel_file = os.path.join(self.root, u.speaker, f'{u.feature_file}.npy')
            wav_file = os.path.join(self.root, u.speaker, f'{u.feature_file}.wav')
            try:
                np.save(mel_file, mel)
                write_wav_int16(wav_file, self.fs, wav)
                self.written += 1
            except Exception as e:
                _logger.error(f'{u.feature_dir} -- {u.feature_file} -- {e}')
                for path in (mel_file, wav_file):
                    if os.path.isfile(path):
                        os.remove(path)


def fine_tuning(hparams):
    ''' Extract mel-specs and audio files for Vocoder fine-tuning (`fine_tune.py:23-123`).  Returns counts and host timings
        {'utterances', 'written', 'skipped', 'seconds', 'read_wait_s', 'write_s'}. '''
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    model = DaftExprt(hparams).cuda(0)
    if not hparams.checkpoint:
        raise ValueError(f'No checkpoint specified -- "{hparams.checkpoint}"')
    checkpoint_dict = torch.load(hparams.checkpoint, map_location='cpu', weights_only=False)
    model.load_state_dict({k.replace('module.', ''): v for k, v in checkpoint_dict['state_dict'].items()})

    hparams.multiprocessing_distributed = False
    train_loader, _, _, _ = prepare_data_loaders(hparams, num_workers=0, drop_last=False, distributed=False)

    ft_data_set = os.path.join(os.path.dirname(hparams.training_files), 'fine_tuning_dataset')
    hparams.ft_data_set = ft_data_set
    for speaker in hparams.speakers:
        os.makedirs(os.path.join(ft_data_set, speaker), exist_ok=True)

    fs, n_mel = int(hparams.sampling_rate), int(hparams.n_mel_channels)
    model.eval()
    start, read_wait, n_utts = time.time(), 0., 0
    files = _PackedFiles(hparams, ft_data_set)
    writer = WriteBehind(files, 'fine_tune_writer')
    reader = ThreadPoolExecutor(max_workers=1, thread_name_prefix='fine_tune_reader')
    try:
        with torch.no_grad():
            for idx, batch in enumerate(train_loader):
                inputs, _, (feature_dirs, feature_files) = model.parse_batch(0, batch)
                pending = reader.submit(_read_batch, hparams, feature_dirs, feature_files)
                _, _, _, (mel_specs, output_lengths), _ = model(inputs)
                t0 = time.time()
                utts = pending.result()
                read_wait += time.time() - t0
                wavs, n_total = device_waves(utts, fs, dev)
                lengths = [int(t) for t in batch[9]]
                crops = [crop_range(u.span[0], u.span[1], fs, n) for u, n in zip(utts, n_total)]
                for u, (_, n), T in zip(utts, crops, lengths):
                    if nb_frames(n, hparams) != T:
                        raise ValueError(f'{u.feature_dir} -- {u.feature_file}: the cropped audio gives {nb_frames(n, hparams)} '
                                         f'frames, the mel prediction has {T}')
                crop = torch.tensor(crops, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
                buf = ft_pack(mel_specs, output_lengths, wavs, crop, n_mel * sum(lengths), sum(n for _, n in crops))
                writer.put(buf, utts, crops, lengths)
                n_utts += len(utts)
                if idx % 10 == 0 or idx == len(train_loader) - 1:
                    _logger.info(f'fine-tuning data set: batch {idx + 1} / {len(train_loader)}, {n_utts} utterances, '
                                 f'{time.time() - start:.1f} s')
    finally:
        reader.shutdown(wait=True)
        writer.close()
    torch.cuda.synchronize()
    return {'utterances': n_utts, 'written': files.written, 'skipped': files.skipped, 'seconds': time.time() - start,
            'read_wait_s': read_wait, 'write_s': writer.busy_s}


def launch_fine_tuning(data_set_dir, config_file, log_file):
    ''' `fine_tune.py:126-168` '''
    logging.basicConfig(handlers=[logging.StreamHandler(), logging.FileHandler(log_file)],
                        format='%(asctime)s [%(levelname)s] %(message)s', datefmt='%Y-%m-%d %H:%M:%S', level=logging.INFO)
    with open(config_file) as f:
        config = json.load(f)
    hparams = HyperParams(verbose=False, **config)
    hparams.data_set_dir = data_set_dir
    hparams.config_file = config_file
    hparams.save_hyper_params(hparams.config_file)
    torch.manual_seed(0)
    _logger.info(f'PyTorch version -- {torch.__version__}')
    _logger.info(f'HIP version -- {torch.version.hip}\n')
    fine_tuning(hparams)


if __name__ == '__main__':
    parser = argparse.ArgumentParser()
    parser.add_argument('--data_set_dir', type=str, required=True, help='Data set containing .wav files')
    parser.add_argument('--config_file', type=str, required=True,
                        help='JSON configuration file to initialize hyper-parameters for fine-tuning')
    parser.add_argument('--log_file', type=str, required=True, help='path to save logger outputs')
    args = parser.parse_args()
    launch_fine_tuning(args.data_set_dir, args.config_file, args.log_file)
