"""Batched prosody-transfer synthesis driver.

Keeps the hot-path part of the reference driver (`src/daft_exprt/generate.py`): `collate_tensors` (140-239: symbol ids,
per-symbol duration / energy / pitch control factors, reference `.npz` prosody, sort by symbol count, padding rules),
`generate_batch_mel_specs` (242-317: one `model.inference` call per batch, crop per item, `.npz` with the same keys,
Griffin-Lim preview `.wav` per item on the GPU, `daft_exprt/griffin_lim.py`, or HiFi-GAN audio, `daft_exprt/vocoder.py`) and `generate_mel_specs` (320-437: chunking +
real-time-factor accounting) and `extract_reference_parameters` (440-462: a reference recording -> the `.npz` of energy, pitch
and mel-spectrogram the collate reads; wav reading, resampling, pitch and mel all on the GPU).  Plots are outside the accelerated
path.  The drivers here take sentences phonemised -- a list of words (lists of phone symbols) and boundary
symbols, exactly what `prepare_sentences_for_inference` returns; `phonemize_sentence` and `prepare_sentences_for_inference`
(28-107, 465-494) are those of `daft_exprt/text.py`, re-exported here under the reference's import path: a dictionary lookup, and a
g2p model trained on that dictionary (`daft_exprt/g2p.py`) in place of `mfa g2p`.
"""
import logging
import os
import time
from types import SimpleNamespace

import numpy as np
import torch

from daft_exprt import _hip as H
from daft_exprt import audio, evaluate, griffin_lim
from daft_exprt.recordings import _parameters_of, waves_to_device
from daft_exprt.text import phonemize_sentence, prepare_sentences_for_inference  # noqa: F401
from daft_exprt.vocoder import pcm16

_logger = logging.getLogger(__name__)


def chunker(seq, size):
    ''' successive chunks of `size` items (`utils.py:92`) '''
    return [seq[pos: pos + size] for pos in range(0, len(seq), size)]


def _symbol_ids(sentence, hparams):
    ids = []
    for item in sentence:
        if isinstance(item, (list, tuple)):      # phones of one word
            ids.extend(hparams.symbols.index(phone) for phone in item)
        else:                                     # word boundary / punctuation / eos
            ids.append(hparams.symbols.index(item))
    return ids


def collate_tensors(batch_sentences, batch_dur_factors, batch_energy_factors, batch_pitch_factors, pitch_transform,
                    batch_refs, batch_speaker_ids, batch_file_names, hparams):
    ''' same contract as `generate.py:140-239`; `batch_refs` are `.npz` paths (keys energy, pitch, mel_spec),
        already-loaded (energy, pitch, mel_spec) triples, or `.wav` paths whose parameters are extracted on the fly '''
    assert pitch_transform in ('add', 'multiply')
    neutral_pitch = 0. if pitch_transform == 'add' else 1.
    rows = []
    for sentence, dur_f, en_f, pi_f, ref in zip(batch_sentences, batch_dur_factors, batch_energy_factors, batch_pitch_factors, batch_refs):
        ids = _symbol_ids(sentence, hparams)
        n = len(ids)
        dur_f = [1.] * n if dur_f is None else list(dur_f)
        en_f = [1.] * n if en_f is None else list(en_f)
        pi_f = [neutral_pitch] * n if pi_f is None else list(pi_f)
        assert len(dur_f) == n, _logger.error(f'{len(dur_f)} duration factors whereas there a {n} symbols')
        assert len(en_f) == n, _logger.error(f'{len(en_f)} energy factors whereas there a {n} symbols')
        assert len(pi_f) == n, _logger.error(f'{len(pi_f)} pitch factors whereas there a {n} symbols')
        if _is_wav(ref):
            ref = reference_parameters([ref], hparams)[0]
        elif isinstance(ref, (str, os.PathLike)):
            data = np.load(ref)
            ref = (data['energy'], data['pitch'], data['mel_spec'])
        energy, pitch, mel = (torch.as_tensor(np.asarray(a)).float() for a in ref)
        rows.append((torch.tensor(ids, dtype=torch.long), torch.tensor(dur_f), torch.tensor(en_f), torch.tensor(pi_f), energy, pitch, mel))
    n = len(rows)
    input_lengths, order = torch.sort(torch.LongTensor([len(r[0]) for r in rows]), dim=0, descending=True)
    L, T = int(input_lengths[0]), max(r[6].size(1) for r in rows)
    symbols = torch.zeros(n, L, dtype=torch.long)
    dur_factors, energy_factors = torch.ones(n, L), torch.ones(n, L)
    pitch_factors = torch.full((n, L), neutral_pitch)
    energy_refs, pitch_refs = torch.zeros(n, T), torch.zeros(n, T)
    mel_spec_refs = torch.zeros(n, hparams.n_mel_channels, T)
    ref_lengths, speaker_ids, file_names = torch.zeros(n, dtype=torch.long), torch.zeros(n, dtype=torch.long), []
    for row, src in enumerate(order.tolist()):
        ids, dur_f, en_f, pi_f, energy, pitch, mel = rows[src]
        l, t = len(ids), mel.size(1)
        symbols[row, :l], dur_factors[row, :l], energy_factors[row, :l], pitch_factors[row, :l] = ids, dur_f, en_f, pi_f
        energy_refs[row, :t], pitch_refs[row, :t], mel_spec_refs[row, :, :t] = energy, pitch, mel
        ref_lengths[row], speaker_ids[row] = t, batch_speaker_ids[src]
        file_names.append(batch_file_names[src])
    return symbols, dur_factors, energy_factors, pitch_factors, input_lengths, energy_refs, pitch_refs, mel_spec_refs, \
        ref_lengths, speaker_ids, file_names


def _is_wav(ref):
    return isinstance(ref, (str, os.PathLike)) and str(ref).lower().endswith('.wav')


def _ref_name(ref, idx):
    ''' `_ref_<basename without .npz>` part of the output file name (`generate.py:250-251`); references handed over as
        already-loaded triples (an extension, the reference only takes paths) are named by their position, `.wav`
        references (an extension too) by their basename without `.wav` '''
    if _is_wav(ref):
        return os.path.basename(str(ref))[:-len('.wav')]
    if isinstance(ref, (str, os.PathLike)):
        return os.path.basename(str(ref)).replace('.npz', '')
    return f'mem{idx}'


def generate_batch_mel_specs(model, batch_sentences, batch_refs, batch_dur_factors, batch_energy_factors, batch_pitch_factors,
                             pitch_transform, batch_speaker_ids, batch_file_names, output_dir, hparams, n_jobs=1,
                             use_griffin_lim=True, scores=None, vocoder=None, prosody_targets=None, recognizer=None,
                             intelligibility=None, speaker_encoder=None, speaker_identity=None):
    ''' `generate.py:242-317`, same contract: every file name gets the `_spk_<id>_ref_<reference>` suffix IN PLACE
        (the caller's list is updated like the reference does, 248-253), one `model.inference` call on the collated
        batch, `<output_dir>/<file_name>.npz` holding `mel_spec` (298), and the return value
        `{file_name: [duration, duration_int, energy, pitch, mel_spec, alignment]}` cropped per item (300).
        With `use_griffin_lim` (303-307, 110-137) the preview audio is made on the device from the decoder's mel before the
        copy to the host (`griffin_lim.griffin_lim_batch`, 30 iterations, device noise seeded with 0) and written as
        `<output_dir>/<file_name>.wav`: mono, `hparams.sampling_rate`, 64-bit float, peak 1.  Plots stay outside the
        accelerated path.
        `scores` (an extension; needs `use_griffin_lim` or `vocoder`): a dict that receives, per file name, the prosody-transfer scores of
        the generated audio against its reference (`evaluate.prosody_transfer_scores`, computed on the device beside the audio):
        `pitch_pcc`, `energy_pcc` (floats, NaN where undefined), `voiced_ref`, `voiced_gen`, `frames_ref`, `frames_gen` (ints).
        With None nothing is computed and nothing else changes.
        `vocoder` (an extension): a `vocoder.Vocoder` (HiFi-GAN generator).  `<file_name>.wav` is then the vocoder's audio of the
        decoder's mel, made on the device before the copy to the host and written as 16-bit PCM (`audio.write_wav_int16`,
        `n_frames * hop` samples); `use_griffin_lim` is not needed and no preview is made; `scores` are computed on the vocoder's
        audio.  With None nothing changes.
        `prosody_targets` (an extension): per sentence, in the caller's order, None or a one-row `clone.ProsodyTargets`
        of that sentence's symbols: per-symbol durations (frames), energies and pitches imposed on the predictions; raw units are
        standardised with the sentence's speaker.  The collate's sort is applied to them.  With None nothing changes.
        `recognizer` (an extension; needs `use_griffin_lim` or `vocoder`): a `recognizer.Recognizer`.  The dict
        `intelligibility` then receives, per file name, the phone error rate of the generated audio against the phones that were
        asked for (`recognizer.audio_error_rates`, on the device beside the audio): sub, del, ins, n_ref, per (NaN without a
        reference phone) and n_hyp.  With None nothing is computed and nothing else changes.
        `speaker_encoder` (an extension; needs `use_griffin_lim` or `vocoder`): a `speaker.SpeakerEncoder` with centroids.
        The dict `speaker_identity` then receives, per file name: `speaker_id` (the speaker that was asked for), `reference` (the
        reference's name), `reference_identified_as` (the speaker whose centroid the REFERENCE recording's mel is nearest to), and
        `speaker.audio_speaker_scores` of the generated audio against the requested speaker -- cos_target, margin, identified,
        accepted -- with cos_reference, the cosine to the embedding of the reference recording itself.  With None nothing is
        computed and nothing else changes. '''
    source = 'vocoder' if vocoder is not None else 'griffin_lim' if use_griffin_lim else None
    if scores is not None and source is None:
        raise ValueError('scores are computed from generated audio: pass use_griffin_lim=True (the Griffin-Lim preview) or a vocoder')
    if recognizer is not None and (source is None or intelligibility is None):
        raise ValueError('a recogniser scores generated audio into `intelligibility`: pass that dict, and use_griffin_lim=True or a vocoder')
    if speaker_encoder is not None and (source is None or speaker_identity is None):
        raise ValueError('a speaker encoder scores generated audio into `speaker_identity`: pass that dict, and use_griffin_lim=True or a vocoder')
    reference_of = {}
    for idx, file_name in enumerate(batch_file_names):
        file_name += f'_spk_{batch_speaker_ids[idx]}'
        file_name += f'_ref_{_ref_name(batch_refs[idx], idx)}'
        batch_file_names[idx] = file_name
        reference_of[file_name] = _ref_name(batch_refs[idx], idx)
        _logger.info(f'Generating "{batch_sentences[idx]}" as "{file_name}"')
    col = collate_tensors(batch_sentences, batch_dur_factors, batch_energy_factors, batch_pitch_factors, pitch_transform,
                          batch_refs, batch_speaker_ids, batch_file_names, hparams)
    file_names = col[-1]
    gpu = next(model.parameters()).device
    core = model if hasattr(model, 'check_ids') else getattr(model, 'module', None)
    if core is not None and hasattr(core, 'check_ids'):
        core.check_ids(col[0], col[9], training=False)       # the reference's nn.Embedding would raise IndexError here
    if pitch_transform == 'add':
        for spk in col[9].tolist():
            hparams.stats[f'spk {spk}']['pitch']             # KeyError like `model.py:824-825` when a speaker has no statistics
    inputs = tuple(t.to(gpu, non_blocking=True) for t in col[:-1])
    inference = model.inference if hasattr(model, 'inference') else model.module.inference   # DDP-wrapped callers (270-278)
    targets = None
    if prosody_targets is not None:
        from daft_exprt.clone import ProsodyTargets     # (`clone` imports this module for `_symbol_ids`)
        assert len(prosody_targets) == len(batch_sentences), f'{len(prosody_targets)} prosody targets for {len(batch_sentences)} sentences'
        targets = ProsodyTargets.stack(list(prosody_targets), int(col[4][0]), gpu)
    if targets is None:
        encoder_preds, decoder_preds, alignments = inference(inputs, pitch_transform, hparams)
    else:       # the rows go where `collate_tensors` put their sentences: the same sort of the same symbol counts
        order = torch.sort(torch.LongTensor([len(_symbol_ids(s, hparams)) for s in batch_sentences]), dim=0, descending=True)[1]
        targets = targets.standardised(hparams, list(batch_speaker_ids)).permute(order)
        encoder_preds, decoder_preds, alignments = inference(inputs, pitch_transform, hparams, prosody_targets=targets)
    if source == 'vocoder':              # HiFi-GAN audio, written as 16-bit PCM
        vocoder.check_hparams(hparams)
        wavs, n_samples = vocoder(decoder_preds[0].float().contiguous(), decoder_preds[1])
        samples, write = pcm16(wavs), audio.write_wav_int16
    elif source == 'griffin_lim':        # the Griffin-Lim preview, written as 64-bit float
        wavs, n_samples = griffin_lim.griffin_lim_batch(decoder_preds[0].float().contiguous(), decoder_preds[1], hparams)
        samples, write = wavs, audio.write_wav
    if source is not None:
        if scores is not None:
            batch_scores = evaluate.prosody_transfer_scores(wavs, n_samples, inputs[6], inputs[5], inputs[8], hparams)
        if recognizer is not None:
            from daft_exprt.recognizer import PER_KEYS, audio_error_rates, per_to_host
            batch_per = audio_error_rates(recognizer, wavs, n_samples, inputs[0], inputs[4], hparams)
        if speaker_encoder is not None:
            from daft_exprt.speaker import audio_speaker_scores, nearest_speakers, scores_to_host
            with torch.no_grad():
                reference_embeddings = speaker_encoder.embed(inputs[7].float(), inputs[8])
            batch_spk = audio_speaker_scores(speaker_encoder, wavs, n_samples, inputs[9], hparams, reference_embeddings)
            reference_speakers = nearest_speakers(speaker_encoder, reference_embeddings)
    duration, duration_int, energy, pitch, input_lengths = (t.detach().cpu().numpy() for t in encoder_preds)
    mel_spec, output_lengths = (t.detach().cpu().numpy() for t in decoder_preds)
    weights = alignments.detach().cpu().numpy()
    predictions = {}
    for i in range(mel_spec.shape[0]):
        l, t = int(input_lengths[i]), int(output_lengths[i])
        name = file_names[i]
        np.savez(os.path.join(output_dir, f'{name}.npz'), mel_spec=mel_spec[i, :, :t])
        predictions[f'{name}'] = [duration[i, :l], duration_int[i, :l], energy[i, :l], pitch[i, :l], mel_spec[i, :, :t],
                                  weights[i, :l, :t]]
    if source is not None:
        samples, n_samples = samples.cpu().numpy(), n_samples.cpu().numpy()
        for i, name in enumerate(file_names):
            write(os.path.join(output_dir, f'{name}.wav'), hparams.sampling_rate, samples[i, :int(n_samples[i])])
        if scores is not None:
            host = {key: t.cpu().tolist() for key, t in batch_scores.items()}
            for i, name in enumerate(file_names):
                scores[name] = {key: host[key][i] for key in evaluate.SCORE_KEYS}
        if recognizer is not None:
            host = per_to_host(batch_per)
            for i, name in enumerate(file_names):
                intelligibility[name] = {key: host[key][i] for key in PER_KEYS}
        if speaker_encoder is not None:
            host, requested = scores_to_host(batch_spk), inputs[9].cpu().tolist()
            for i, name in enumerate(file_names):
                speaker_identity[name] = {'speaker_id': requested[i], 'reference': reference_of[name],
                                          'reference_identified_as': reference_speakers[i], **{key: host[key][i] for key in host}}
        _logger.warning('Mel-spec / alignment plots are outside the accelerated path')
    return predictions


def reference_parameters(audio_refs, hparams, device=None):
    ''' [(energy, pitch, mel_spec)] of wav files, in order: read on the host and brought to hparams.sampling_rate on the device
        (`recordings.waves_to_device`), then tracked and analysed there as one batch (`recordings._parameters_of`) '''
    wavs, lengths = waves_to_device([SimpleNamespace(wav_file=path) for path in audio_refs], int(hparams.sampling_rate), H.device(device))
    return _parameters_of(wavs, lengths, hparams)


def _ref_file(audio_ref, output_dir):
    return os.path.join(output_dir, os.path.basename(audio_ref).replace('.wav', '') + '.npz')


def extract_reference_parameters(audio_ref, output_dir, hparams, device=None):
    ''' `generate.py:440-462`, same contract: `<output_dir>/<name of audio_ref without .wav>.npz` with keys `energy`, `pitch`
        (log Hz per mel frame, 0 where unvoiced) and `mel_spec`, all of the same number of frames; nothing is done when the
        file already exists.  The batch form with one file: the energy is the front-end's own (the norm of exp(mel) over the
        channels, what `extract_energy(np.exp(mel_spec))` computes). '''
    extract_reference_parameters_batch([audio_ref], output_dir, hparams, device)


def extract_reference_parameters_batch(audio_refs, output_dir, hparams, device=None):
    ''' `extract_reference_parameters` for a whole style bank: the files that have no `.npz` yet go through one resampling
        launch per source rate, one pitch track and one mel front-end call together (`reference_parameters`) '''
    os.makedirs(output_dir, exist_ok=True)
    todo = [ref for ref in audio_refs if not os.path.isfile(_ref_file(ref, output_dir))]
    todo = list(dict.fromkeys(todo))
    if not todo:
        return
    for ref, (energy, pitch, mel_spec) in zip(todo, reference_parameters(todo, hparams, device)):
        np.savez(_ref_file(ref, output_dir), energy=energy, pitch=pitch, mel_spec=mel_spec)


def read_phonemised_sentences(path, symbols=None):
    ''' (sentences, file_names) of a file in the format `prepare_sentences_for_inference` writes (`generate.py:483-492`,
        `sentences_to_generate.txt`): one `file_name|{P1 P2} {P3} , {P4} ? ~` per line.  A brace group is a word (a list of
        phones), a bare token a boundary symbol, two adjacent words are separated by the whitespace symbol the writer's
        whitespace collapse swallowed, a trailing `~` is the eos.  `symbols`: the table every phone and boundary must be in
        (default: the English one); anything else raises ValueError naming the line. '''
    import re
    from daft_exprt.symbols import symbols_english, whitespace
    table = set(symbols_english if symbols is None else symbols)
    sentences, file_names = [], []
    with open(path, 'r', encoding='utf-8') as f:
        lines = [line.strip() for line in f]
    for number, line in enumerate(lines, 1):
        if not line:
            continue
        where = f'{path}, line {number}'
        if '|' not in line:
            raise ValueError(f'{where}: expected "file_name|phonemised sentence", got "{line}"')
        file_name, text = line.split('|', 1)
        if re.sub(r'\{[^{}]*\}', '', text).count('{') or re.sub(r'\{[^{}]*\}', '', text).count('}'):
            raise ValueError(f'{where}: unbalanced braces in "{text}"')
        sentence = []
        for group, token in re.findall(r'\{([^{}]*)\}|(\S+)', text):
            if token:
                if token not in table:
                    raise ValueError(f'{where}: unknown symbol "{token}"')
                sentence.append(token)
                continue
            phones = group.split()
            unknown = [phone for phone in phones if phone not in table]
            if unknown or not phones:
                raise ValueError(f'{where}: unknown symbol "{unknown[0]}"' if unknown else f'{where}: empty word')
            if sentence and isinstance(sentence[-1], list):
                sentence.append(whitespace)
            sentence.append(phones)
        if not sentence:
            raise ValueError(f'{where}: no symbols')
        sentences.append(sentence)
        file_names.append(file_name)
    return sentences, file_names


LAST_TIME_PERF = {}   # filled by generate_mel_specs(get_time_perf=True): what the reference only logs (generate.py:433-435)


def generate_mel_specs(model, sentences, file_names, speaker_ids, refs, output_dir, hparams, dur_factors=None,
                       energy_factors=None, pitch_factors=None, batch_size=1, n_jobs=1, use_griffin_lim=False,
                       get_time_perf=False, scores=None, vocoder=None, prosody_targets=None, recognizer=None, intelligibility=None,
                       speaker_encoder=None, speaker_identity=None):
    ''' `generate.py:320-437`, same contract: `pitch_factors = [transform, [per-sentence factor lists]]`, the list-length
        asserts, eval mode + no grad, chunks of `batch_size`, returns the predictions dict only.  With `get_time_perf`
        the real-time factor is logged exactly like the reference: wall time of the whole per-batch function (collate,
        H2D, inference, D2H, file writes) against `((n_frames - 1) * hop + n_fft - 2 * (n_fft // 2)) / sr` seconds of
        audio per sentence (413-435); the numbers are also left in `LAST_TIME_PERF`.  `scores`, `vocoder`,
        `prosody_targets` (one entry per sentence, in the caller's order), `recognizer` and `intelligibility`, `speaker_encoder`
        and `speaker_identity`: see `generate_batch_mel_specs`. '''
    if scores is not None and not use_griffin_lim and vocoder is None:
        raise ValueError('scores are computed from generated audio: pass use_griffin_lim=True (the Griffin-Lim preview) or a vocoder')
    n = len(sentences)
    dur_factors = [None for _ in range(n)] if dur_factors is None else dur_factors
    energy_factors = [None for _ in range(n)] if energy_factors is None else energy_factors
    pitch_factors = ['add', [None for _ in range(n)]] if pitch_factors is None else pitch_factors
    pitch_transform = pitch_factors[0].lower()
    pitch_factors = pitch_factors[1]
    assert pitch_transform in ['add', 'multiply'], _logger.error(f'Pitch transform "{pitch_transform}" is not currently supported')
    for what, seq in (('filenames', file_names), ('speaker IDs', speaker_ids), ('references', refs),
                      ('duration factors', dur_factors), ('energy factors', energy_factors), ('pitch factors', pitch_factors)):
        assert len(seq) == n, _logger.error(f'{len(seq)} {what} but there are {n} sentences to generate')
    if prosody_targets is not None:
        assert len(prosody_targets) == n, _logger.error(f'{len(prosody_targets)} prosody targets but there are {n} sentences to generate')
    model.eval()
    os.makedirs(output_dir, exist_ok=True)
    predictions, time_per_batch = {}, []
    with torch.no_grad():
        for chunk in zip(chunker(sentences, batch_size), chunker(refs, batch_size), chunker(dur_factors, batch_size),
                         chunker(energy_factors, batch_size), chunker(pitch_factors, batch_size),
                         chunker(speaker_ids, batch_size), chunker(file_names, batch_size),
                         chunker([None] * n if prosody_targets is None else list(prosody_targets), batch_size)):
            b_sent, b_refs, b_dur, b_en, b_pi, b_spk, b_names, b_targets = chunk
            begin = time.time() if get_time_perf else None
            extra = () if prosody_targets is None else (b_targets,)         # (without targets the call is the one it always was)
            more = {} if recognizer is None else {'recognizer': recognizer, 'intelligibility': intelligibility}
            if speaker_encoder is not None:
                more.update(speaker_encoder=speaker_encoder, speaker_identity=speaker_identity)
            predictions.update(generate_batch_mel_specs(model, b_sent, b_refs, b_dur, b_en, b_pi, pitch_transform, b_spk,
                                                        b_names, output_dir, hparams, n_jobs, use_griffin_lim, scores, vocoder, *extra,
                                                        **more))
            time_per_batch += [time.time() - begin] if get_time_perf else []
    if get_time_perf:
        durations = []
        for prediction in predictions.values():
            nb_frames = prediction[4].shape[1]
            nb_wav_samples = (nb_frames - 1) * hparams.hop_length + hparams.filter_length
            if hparams.centered:
                nb_wav_samples -= 2 * int(hparams.filter_length / 2)
            durations.append(nb_wav_samples / hparams.sampling_rate)
        LAST_TIME_PERF.clear()
        LAST_TIME_PERF.update({'sentences': len(predictions), 'audio_seconds': sum(durations), 'wall_seconds': sum(time_per_batch),
                               'rtf': sum(durations) / sum(time_per_batch)})
        _logger.info('')
        _logger.info(f'{len(predictions)} sentences ({sum(durations):.2f}s) generated in {sum(time_per_batch):.2f}s')
        _logger.info(f'DaftExprt RTF: {sum(durations) / sum(time_per_batch):.2f}')
    return predictions
