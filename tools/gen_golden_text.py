#!/usr/bin/env python
"""Record tests/golden/text_frontend.json by IMPORTING the reference (`/root/reference/src/daft_exprt`) in the build container:
what its `cleaners.text_cleaner` and `generate.phonemize_sentence` make of a handful of sentences.  Only data is written: the
input sentences, a fabricated dictionary and the recorded outputs.

Shims, all outside the reference tree: stub modules for the absent third-party imports.  `unidecode` is the identity and `inflect`
an engine without methods, so the sentences are ASCII and digit-free -- those two packages are then never consulted.  The
dictionary lists ONE pronunciation for EVERY word of the sentences, so `random.choice` has nothing to choose and `mfa g2p` is never
started.  Every sentence for `phonemize_sentence` ends in a punctuation mark: the reference fails without one.

Run:  python tools/gen_golden_text.py
"""
import json
import os
import re
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = '/root/reference/src'
OUT = os.path.join(ROOT, 'tests', 'golden', 'text_frontend.json')

SENTENCES = [
    "that's, an 'example! ' of a sentence. '",                    # the docstring example of the reference (generate.py:47)
    'Mr. Smith met Dr. Jones and Mrs. Hall at St. Mary, Ltd. today.',     # (an abbreviation swallows its dot: not at the end)
    'A well-known fact -- truly (really) "quoted" -- stands.',
    'Wait... what?! No way!!',
    ', . Hello there , , world !',
    'Semi; colon: and under_score, done...',
    "'Tis the dogs' bone, isn't it?",
    'yes?',
]
CLEAN_ONLY = [
    'No closing mark',
    '  -- leading dashes, and spaces  ',
    'Col. Mustard (in the library) said: "hmm"; Capt. Hook agreed .',
    'one , two ,, three ,',
    'what ?? really !? yes .!',
]
LETTER_PHONES = dict(zip("abcdefghijklmnopqrstuvwxyz'", ['AE1', 'B', 'K', 'D', 'EH1', 'F', 'G', 'HH', 'IH1', 'JH', 'K', 'L', 'M', 'N', 'OW1', 'P', 'K',
                                                         'R', 'S', 'T', 'AH1', 'V', 'W', 'Z', 'Y', 'Z', 'AH0']))


def install_shims():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    import importlib.util
    stub('unidecode', unidecode=lambda s: s)
    stub('inflect', engine=lambda: None)
    for name in ('librosa', 'tgt'):
        if importlib.util.find_spec(name) is None:
            stub(name)
    if 'librosa' in sys.modules and not hasattr(sys.modules['librosa'], 'filters'):
        sys.modules['librosa'].filters = stub('librosa.filters', mel=lambda *a, **k: None)
    sys.path.insert(0, REF_SRC)


def main():
    install_shims()
    from daft_exprt.cleaners import text_cleaner
    from daft_exprt.generate import phonemize_sentence
    for s in SENTENCES + CLEAN_ONLY:
        assert s.isascii() and not re.search(r'[0-9]', s), s
    words = sorted({w for s in SENTENCES for w in re.findall(r"[\w']+", text_cleaner(s.strip(), 'english').lower())})
    dictionary = {w: [LETTER_PHONES[c] for c in w if c in LETTER_PHONES] for w in words}
    dictionary = {w: p for w, p in dictionary.items() if p}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'english.dict')
        with open(path, 'w', encoding='utf-8') as f:
            for w, p in dictionary.items():
                f.write(f'{w} {" ".join(p)}\n')
        hp = types.SimpleNamespace(mfa_dictionary=path, mfa_g2p_model=os.path.join(tmp, 'never_used.zip'), language='english')
        cases = []
        for s in SENTENCES:
            out = phonemize_sentence(s, hp, None)
            assert '<unk>' not in out, (s, out)
            cases.append({'sentence': s, 'cleaned': text_cleaner(s.strip(), 'english'), 'phonemized': out})
    cleaned = [{'text': s, 'cleaned': text_cleaner(s, 'english')} for s in SENTENCES + CLEAN_ONLY]
    with open(OUT, 'w', encoding='utf-8') as f:
        json.dump({'dictionary': dictionary, 'phonemize_sentence': cases, 'text_cleaner': cleaned}, f, indent=1)
    print(f'wrote {OUT}: {len(cases)} sentences, {len(cleaned)} cleaner cases, {len(dictionary)} dictionary words')


if __name__ == '__main__':
    main()
