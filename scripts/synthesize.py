#!/usr/bin/env python
"""Batched prosody-transfer synthesis with objective scores, behind the flags of the reference's `scripts/synthesize.py`:
    python scripts/synthesize.py -out OUT_DIR -chk CHECKPOINT -tf SENTENCES -sb STYLE_BANK [-bs N] [-rtf] [-ctrl] [-voc G_CKPT [-vcfg JSON]]
                                 [-dict DICTIONARY [-g2p G2P_CKPT]] [-rec RECOGNIZER] [-spk SPEAKER_ENCODER]

  -tf   phonemised sentences, one `file_name|{P1 P2} {P3} , {P4} ? ~` per line: the `sentences_to_generate.txt` the reference
        writes after text cleaning and g2p (`generate.read_phonemised_sentences`); with -dict: raw text, one sentence per line
  -dict a pronunciation dictionary (`word P1 P2 ...` per line): -tf is then RAW text, which is cleaned, looked up and written to
        `<out>/sentences_to_generate.txt` first (`generate.prepare_sentences_for_inference`); -g2p: the model of
        `scripts/train_g2p.py` for the words the dictionary lacks (without it such a word is an error)
  -sb   directory of reference `.wav` files; each gets its `.npz` of energy, pitch and mel-spectrogram beside it, extracted on
        the GPU as one batch
  -rtf  an extra pass without audio that logs the real-time factor at this batch size
  -ctrl the reference's control example instead of plain transfer: every symbol 1.25 times longer, pitch shifted by +50 Hz
  -voc  a HiFi-GAN generator checkpoint (`torch.save({'generator': state_dict})`, e.g. one fine-tuned on this project's
        `fine_tuning_dataset`); -vcfg its `config.json` (default: the one beside the checkpoint).  The `.wav` files are then the
        vocoder's audio (16-bit PCM) instead of the Griffin-Lim preview, the scores refer to that audio, and -rtf logs a second
        real-time factor that includes the vocoder
  -rec  a phone recogniser (`scripts/train_recognizer.py`): `<out>/intelligibility.json` then holds, per output file, the
        substitutions, deletions and insertions of the recogniser's decode of the synthesised audio against the phones that were
        asked for, their sum over the reference length (`per`), and the corpus-level rate (summed errors / summed reference
        length).  How that rate tracks listeners has not been measured
  -spk  a speaker encoder (`scripts/train_speaker_encoder.py`): `<out>/speaker_identity.json` then holds, per output file, the
        requested speaker, the reference, the speaker whose centroid the reference RECORDING is nearest to
        (`reference_identified_as`), and of the synthesised audio the cosine to the requested speaker's centroid (`cos_target`),
        its `margin` over the other centroids, whether it is `identified` as and `accepted` for the requested speaker, and the
        cosine to the embedding of the reference recording (`cos_reference`).  The summary has the share identified and, over the
        files whose reference is nearest to another speaker, the mean of cos_target - cos_reference and the share where it is
        negative: the leak of the reference's speaker that the model's adversarial speaker classifier exists to prevent.  How the
        cosines track listeners' judgement of speaker similarity has not been measured

Every sentence gets a random reference of the style bank and a random speaker (`random.seed(1234)`), is synthesised with
Griffin-Lim preview audio and scored on the device against its reference: `<out>/prosody_transfer.json` holds, per output file,
the pitch and energy correlation (`daft_exprt/evaluate.py`; null where undefined) and the frame counts, and a summary with the
mean and median of the defined values and the number of undefined ones, and `"audio"`: which audio was scored ("hifi-gan" with
-voc, else "griffin-lim").  Without -ctrl each preview is renamed to
`<idx>_<name>.wav` and a copy of its reference recording is put beside it as `<idx>_ref.wav`, so that the two sort together."""
import argparse
import json
import logging
import math
import os
import random
import shutil
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')
sys.path.insert(0, PKG)

from daft_exprt import generate  # noqa: E402
from daft_exprt.hparams import HyperParams  # noqa: E402
from daft_exprt.model import DaftExprt  # noqa: E402

_logger = logging.getLogger('synthesize')
CONTROL = {'duration': 1.25, 'pitch': 50.0, 'pitch_transform': 'add'}      # the -ctrl example: slower, and 50 Hz higher
METRICS = ('pitch_pcc', 'energy_pcc')


def load_model(checkpoint):
    ''' (model on cuda:0, the hyper-parameters stored in the checkpoint); `module.` prefixes of data-parallel training are dropped '''
    ckpt = torch.load(checkpoint, map_location='cuda:0', weights_only=False)
    hparams = HyperParams(verbose=False, **ckpt['config_params'])
    weights = {(name[len('module.'):] if name.startswith('module.') else name): t for name, t in ckpt['state_dict'].items()}
    torch.cuda.set_device(0)
    model = DaftExprt(hparams).cuda(0)
    model.load_state_dict(weights)
    return model, hparams


def style_bank(directory, hparams):
    ''' the `.npz` prosody files of the bank, sorted; missing ones are extracted from their `.wav` in one batch '''
    recordings = sorted(f for f in os.listdir(directory) if f.endswith('.wav'))
    generate.extract_reference_parameters_batch([os.path.join(directory, f) for f in recordings], directory, hparams)
    bank = sorted(os.path.join(directory, f) for f in os.listdir(directory) if f.endswith('.npz'))
    if not bank:
        raise SystemExit(f'{directory}: no reference recording (.wav) or prosody file (.npz)')
    return bank


def n_symbols(sentence):
    return sum(len(item) if isinstance(item, (list, tuple)) else 1 for item in sentence)


def load_vocoder(checkpoint, config, hparams):
    ''' the HiFi-GAN generator on cuda:0, checked against the acoustic model's mel front-end '''
    from daft_exprt.vocoder import Vocoder
    vocoder = Vocoder.from_checkpoint(checkpoint, config, compute_dtype=hparams.compute_dtype, device='cuda:0')
    vocoder.check_hparams(hparams)
    return vocoder


def phonemise(args, hparams):
    ''' -dict: the raw text of -tf to `<out>/sentences_to_generate.txt`, which then takes the place of -tf '''
    from daft_exprt.text import load_dictionary
    g2p = None
    if args.g2p is not None:
        from daft_exprt.g2p import load_g2p
        g2p = load_g2p(args.g2p)
    found = {}
    generate.prepare_sentences_for_inference(args.text_file, args.output_dir, hparams, g2p=g2p,
                                             dictionary=load_dictionary(args.dictionary, hparams.symbols), report=found)
    for word, phones in sorted(found['oov'].items()):
        _logger.info(f'not in the dictionary: "{word}" -> {" ".join(phones)}')
    args.text_file = os.path.join(args.output_dir, 'sentences_to_generate.txt')


def run(args, model, hparams, control=None, audio=True, scores=None, vocoder=None, recognizer=None, intelligibility=None,
        speaker_encoder=None, speaker_identity=None):
    ''' one pass over the sentence file; returns [(sentence index, output name, reference .npz)] in sentence order.  With a
        vocoder the audio is its own; `audio` then only decides whether the pass is timed '''
    sentences, names = generate.read_phonemised_sentences(args.text_file, hparams.symbols)
    bank = style_bank(args.style_bank, hparams)
    refs = [random.choice(bank) for _ in sentences]
    speakers = [random.choice(hparams.speakers_id) for _ in sentences]
    dur = pitch = None
    if control is not None:
        dur = [[control['duration']] * n_symbols(s) for s in sentences]
        pitch = [control['pitch_transform'], [[control['pitch']] * n_symbols(s) for s in sentences]]
    os.makedirs(args.output_dir, exist_ok=True)
    more = {} if speaker_encoder is None else {'speaker_encoder': speaker_encoder, 'speaker_identity': speaker_identity}
    predictions = generate.generate_mel_specs(model, sentences, list(names), speakers, refs, args.output_dir, hparams, dur_factors=dur,
                                              pitch_factors=pitch, batch_size=args.batch_size,
                                              use_griffin_lim=audio and vocoder is None, get_time_perf=not audio, scores=scores,
                                              vocoder=vocoder, recognizer=recognizer, intelligibility=intelligibility, **more)
    outputs = []
    for idx, name in enumerate(names):      # the driver returns its own names, a batch at a time in order of length
        mine = [key for key in predictions if key.startswith(f'{name}_spk_{speakers[idx]}_ref_')]
        if len(mine) != 1:
            raise RuntimeError(f'sentence {idx} ("{name}"): expected one output, found {mine}')
        outputs.append((idx, mine[0], refs[idx]))
    return outputs


def pair_with_references(args, outputs):
    ''' {output name: paired name}: `<idx>_<output name>.wav` next to `<idx>_ref.wav`, a copy of the reference recording '''
    paired = {}
    for idx, name, ref in outputs:
        preview = os.path.join(args.output_dir, f'{name}.wav')
        recording = os.path.splitext(ref)[0] + '.wav'
        for path in (preview, recording):
            if not os.path.isfile(path):
                raise FileNotFoundError(path)
        paired[name] = f'{idx}_{name}'
        os.replace(preview, os.path.join(args.output_dir, f'{paired[name]}.wav'))
        shutil.copyfile(recording, os.path.join(args.output_dir, f'{idx}_ref.wav'))
    return paired


def summarise(entries):
    ''' mean and median of the defined values of each correlation, and how many are undefined '''
    summary = {'files': len(entries)}
    for key in METRICS:
        values = [e[key] for e in entries.values() if e[key] is not None]
        summary[key] = {'mean': statistics.fmean(values) if values else None, 'median': statistics.median(values) if values else None,
                        'undefined': len(entries) - len(values)}
    return summary


def write_scores(args, scores, wav_names, audio='griffin-lim'):
    ''' `<out>/prosody_transfer.json`: {'audio': which audio was scored, 'files': {name: scores + 'wav'}, 'summary': ...}; NaN is
        written as null '''
    entries = {}
    for name, values in scores.items():
        entry = {k: (None if isinstance(v, float) and math.isnan(v) else v) for k, v in values.items()}
        entry['wav'] = f'{wav_names.get(name, name)}.wav'
        entries[name] = entry
    report = {'audio': audio, 'files': entries, 'summary': summarise(entries)}
    path = os.path.join(args.output_dir, 'prosody_transfer.json')
    with open(path, 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=1)
    for key in METRICS:
        s = report['summary'][key]
        if s['mean'] is None:
            _logger.info(f'{key}: undefined for all {len(entries)} files')
        else:
            _logger.info(f'{key}: mean {s["mean"]:.3f}, median {s["median"]:.3f} over {len(entries) - s["undefined"]} files '
                         f'({s["undefined"]} undefined)')
    _logger.info(f'Prosody-transfer scores written to {path}')
    return report


def write_intelligibility(args, intelligibility, wav_names, audio='griffin-lim'):
    ''' `<out>/intelligibility.json`: {'audio': which audio was decoded, 'files': {name: sub, del, ins, n_ref, per, n_hyp + 'wav'},
        'summary': the summed counts and 'rate' = summed errors / summed reference length (null without a reference phone)} '''
    entries = {}
    for name, values in intelligibility.items():
        entry = {k: (None if isinstance(v, float) and math.isnan(v) else v) for k, v in values.items()}
        entry['wav'] = f'{wav_names.get(name, name)}.wav'
        entries[name] = entry
    totals = {key: sum(e[key] for e in entries.values()) for key in ('sub', 'del', 'ins', 'n_ref', 'n_hyp')}
    errors = totals['sub'] + totals['del'] + totals['ins']
    report = {'audio': audio, 'files': entries,
              'summary': {'files': len(entries), **totals, 'rate': errors / totals['n_ref'] if totals['n_ref'] else None}}
    path = os.path.join(args.output_dir, 'intelligibility.json')
    with open(path, 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=1)
    _logger.info(f'phone error rate {report["summary"]["rate"]} ({errors} errors over {totals["n_ref"]} phones of {len(entries)} files); '
                 f'written to {path}')
    return report


def write_speaker_identity(args, speaker_identity, wav_names, audio='griffin-lim'):
    ''' `<out>/speaker_identity.json`: {'audio': which audio was embedded, 'files': {name: speaker_id, reference,
        reference_identified_as, cos_target, margin, identified, accepted, cos_reference + 'wav'}, 'summary': files, the shares
        `identified` as and `accepted` for the requested speaker, and over the `other_reference` files whose reference recording is
        nearest to ANOTHER speaker's centroid: `target_minus_reference`, the mean of cos_target - cos_reference, and `leaked`, the
        share where it is negative -- the synthesis is closer to the reference's voice than to the requested one (both null
        without such a file)} '''
    entries = {}
    for name, values in speaker_identity.items():
        entry = {k: (None if isinstance(v, float) and math.isnan(v) else v) for k, v in values.items()}
        entry['wav'] = f'{wav_names.get(name, name)}.wav'
        entries[name] = entry
    other = [e['cos_target'] - e['cos_reference'] for e in entries.values()
             if e['reference_identified_as'] != e['speaker_id'] and e['cos_target'] is not None and e['cos_reference'] is not None]
    summary = {'files': len(entries),
               'identified': sum(e['identified'] for e in entries.values()) / len(entries) if entries else None,
               'accepted': sum(e['accepted'] for e in entries.values()) / len(entries) if entries else None,
               'other_reference': len(other), 'target_minus_reference': statistics.fmean(other) if other else None,
               'leaked': sum(d < 0 for d in other) / len(other) if other else None}
    report = {'audio': audio, 'files': entries, 'summary': summary}
    path = os.path.join(args.output_dir, 'speaker_identity.json')
    with open(path, 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=1)
    _logger.info(f'identified as the requested speaker: {summary["identified"]} of {len(entries)} files; with a reference of another '
                 f'speaker ({len(other)} files): cos_target - cos_reference {summary["target_minus_reference"]}, leaked '
                 f'{summary["leaked"]}; written to {path}')
    return report


def main():
    parser = argparse.ArgumentParser(description='Synthesise phonemised sentences with prosody transferred from a style bank, and score the transfer')
    parser.add_argument('-out', '--output_dir', required=True, help='where the .npz, .wav and prosody_transfer.json go')
    parser.add_argument('-chk', '--checkpoint', required=True, help='training checkpoint (weights and hyper-parameters)')
    parser.add_argument('-tf', '--text_file', required=True, help='phonemised sentences: file_name|{P1 P2} {P3} , {P4} ? ~ per line')
    parser.add_argument('-sb', '--style_bank', required=True, help='directory of reference recordings (.wav)')
    parser.add_argument('-bs', '--batch_size', type=int, default=50, help='sentences per inference call')
    parser.add_argument('-rtf', '--real_time_factor', action='store_true', help='first time a pass without audio and log its real-time factor')
    parser.add_argument('-ctrl', '--control', action='store_true', help='apply the duration x 1.25, pitch + 50 Hz example to every symbol')
    parser.add_argument('-voc', '--vocoder', default=None, help='HiFi-GAN or BigVGAN generator checkpoint: write and score its audio instead of the Griffin-Lim preview')
    parser.add_argument('-vcfg', '--vocoder_config', default=None, help='its config.json (default: beside the vocoder checkpoint)')
    parser.add_argument('-dict', '--dictionary', default=None, help='pronunciation dictionary: -tf is then raw text and is phonemised first')
    parser.add_argument('-g2p', '--g2p', default=None, help='g2p model (scripts/train_g2p.py) for the words the dictionary lacks; needs -dict')
    parser.add_argument('-rec', '--recognizer', default=None, help='phone recogniser (scripts/train_recognizer.py): write intelligibility.json')
    parser.add_argument('-spk', '--speaker_encoder', default=None,
                        help='speaker encoder (scripts/train_speaker_encoder.py): write speaker_identity.json')
    args = parser.parse_args()
    if args.g2p is not None and args.dictionary is None:
        parser.error('-g2p needs -dict')
    logging.basicConfig(format='%(asctime)s [%(levelname)s] %(message)s', datefmt='%Y-%m-%d %H:%M:%S', level=logging.INFO)
    random.seed(1234)

    model, hparams = load_model(args.checkpoint)
    if args.dictionary is not None:
        phonemise(args, hparams)
    vocoder = load_vocoder(args.vocoder, args.vocoder_config, hparams) if args.vocoder else None
    if args.real_time_factor:
        run(args, model, hparams, audio=False)
        if vocoder is not None:
            run(args, model, hparams, audio=False, vocoder=vocoder)
            _logger.info(f'DaftExprt + HiFi-GAN RTF: {generate.LAST_TIME_PERF["rtf"]:.2f}')
    recognizer = None
    if args.recognizer is not None:
        from daft_exprt.recognizer import load_recognizer
        recognizer = load_recognizer(args.recognizer)
    speaker_encoder = None
    if args.speaker_encoder is not None:
        from daft_exprt.speaker import load_speaker_encoder
        speaker_encoder = load_speaker_encoder(args.speaker_encoder)
    scores, intelligibility, speaker_identity = {}, {}, {}
    outputs = run(args, model, hparams, control=CONTROL if args.control else None, scores=scores, vocoder=vocoder,
                  recognizer=recognizer, intelligibility=intelligibility, speaker_encoder=speaker_encoder,
                  speaker_identity=speaker_identity)
    wav_names = {} if args.control else pair_with_references(args, outputs)
    which = 'hifi-gan' if vocoder is not None else 'griffin-lim'
    write_scores(args, scores, wav_names, audio=which)
    if recognizer is not None:
        write_intelligibility(args, intelligibility, wav_names, audio=which)
    if speaker_encoder is not None:
        write_speaker_identity(args, speaker_identity, wav_names, audio=which)


if __name__ == '__main__':
    main()
