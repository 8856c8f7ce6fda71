#!/usr/bin/env python
"""Phonemise raw text with a pronunciation dictionary and a g2p model trained on it
    python scripts/phonemize.py -tf TEXT -dict DICTIONARY -g2p G2P.pt -out OUT_DIR [-lg english]

  -tf    one sentence per line, or `name|sentence` per line (the transcripts of a corpus under their own names)
  -dict  pronunciation dictionary: `word P1 P2 ...` per line
  -g2p   model of `scripts/train_g2p.py` for the words the dictionary lacks; without it such a word is an error
  -out   directory that receives `sentences_to_generate.txt` -- one `file_name|{P1 P2} {P3} , {P4} ? ~` per line, what
         `scripts/synthesize.py`, `scripts/align.py` and `scripts/train_aligner.py` read -- and `phonemize_report.json`

The text is cleaned and split as the reference does (`daft_exprt/text.py`).  The report lists every word that was not in the
dictionary with the transcription the g2p model gave it -- read those; words found in the dictionary are only counted."""
import argparse
import json
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')
sys.path.insert(0, PKG)

_logger = logging.getLogger('phonemize')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Phonemise raw text with a dictionary and a g2p model')
    parser.add_argument('-tf', '--text_file', required=True, help='raw text: one sentence, or name|sentence, per line')
    parser.add_argument('-dict', '--dictionary', required=True, help='pronunciation dictionary: word P1 P2 ... per line')
    parser.add_argument('-g2p', '--g2p', default=None, help='g2p model for the words the dictionary lacks')
    parser.add_argument('-out', '--output_dir', required=True, help='where sentences_to_generate.txt and phonemize_report.json go')
    parser.add_argument('-lg', '--language', type=str, default='english', help='language of the symbol set')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format='%(asctime)s [%(levelname)s] %(message)s', datefmt='%Y-%m-%d %H:%M:%S', level=logging.INFO)
    for flag, path in (('-tf', args.text_file), ('-dict', args.dictionary), ('-g2p', args.g2p)):
        if path is not None and not os.path.isfile(path):
            raise SystemExit(f'phonemize.py: no such file for {flag}: {path}')
    from daft_exprt.hparams import HyperParams
    from daft_exprt.text import load_dictionary, prepare_sentences_for_inference
    hparams = HyperParams(verbose=False, training_files='none', validation_files='none', output_directory=args.output_dir,
                          language=args.language, speakers=['none'])
    dictionary = load_dictionary(args.dictionary, hparams.symbols)
    g2p = None
    if args.g2p is not None:
        from daft_exprt.g2p import load_g2p
        g2p = load_g2p(args.g2p)
    found = {}
    sentences, names = prepare_sentences_for_inference(args.text_file, args.output_dir, hparams, g2p=g2p, dictionary=dictionary,
                                                       report=found)
    report = {'sentences': len(sentences), 'file': os.path.join(args.output_dir, 'sentences_to_generate.txt'),
              'dictionary_words': found['dictionary_words'], 'oov': {w: ' '.join(p) for w, p in sorted(found['oov'].items())}}
    path = os.path.join(args.output_dir, 'phonemize_report.json')
    with open(path, 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=1)
    _logger.info(f'{len(sentences)} sentences written to {report["file"]}: {report["dictionary_words"]} words from the dictionary, '
                 f'{len(report["oov"])} transcribed by the g2p model (listed in {path})')
    return report


if __name__ == '__main__':
    main()
