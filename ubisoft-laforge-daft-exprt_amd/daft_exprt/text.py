"""The text front end: from a raw sentence to the phonemised form the model takes.

Host-side restatement of the reference's `cleaners.py`, `normalize_numbers.py` and of `generate.phonemize_sentence` /
`prepare_sentences_for_inference` (`generate.py:28-107, 465-494`).  Words are looked up in a pronunciation dictionary; the words it
lacks go to a `g2p.G2P` trained on that dictionary (the reference starts `mfa g2p` for them).  Nothing here touches the GPU except
that model.
"""
import os
import re
import unicodedata

from daft_exprt.symbols import eos, punctuation, symbols_english, whitespace


# ---- the dictionary ----------------------------------------------------------------------------------------------------------------------

def load_dictionary(path, symbols=None):
    ''' `{word: [phones, ...]}` with lower-cased keys, as `generate.py:35-39` builds it: one `word P1 P2 ...` per line (the
        Montreal Forced Aligner's format), every line of a word one more pronunciation, in file order.  CMUdict's variant marks
        (`word(2) P1 P2 ...`) are dropped from the key, its `;;;` comment lines and empty lines are skipped, and a pronunciation
        listed twice for a word is kept once.  `symbols`: the table every phone must be in (default: the English one, pass
        `hparams.symbols`); a phone outside it, or a word without phones, raises ValueError naming the line. '''
    table = set(symbols_english if symbols is None else symbols)
    out = {}
    with open(path, 'r', encoding='utf-8') as f:
        for number, line in enumerate(f, 1):
            fields = line.strip().split()
            if not fields or fields[0].startswith(';;;'):
                continue
            word, phones = re.sub(r'\(\d+\)$', '', fields[0]).lower(), fields[1:]
            if not phones or not word:
                raise ValueError(f'{path}, line {number}: no pronunciation for "{fields[0]}"')
            unknown = [p for p in phones if p not in table]
            if unknown:
                raise ValueError(f'{path}, line {number}: unknown phone "{unknown[0]}" for "{fields[0]}"')
            prons = out.setdefault(word, [])
            if phones not in prons:
                prons.append(phones)
    return out


# ---- numbers (normalize_numbers.py) ------------------------------------------------------------------------------------------------------

_UNITS = ('zero one two three four five six seven eight nine ten eleven twelve thirteen fourteen fifteen sixteen seventeen eighteen '
          'nineteen').split()
_TENS = ' ten twenty thirty forty fifty sixty seventy eighty ninety'.split(' ')
_SCALES = ('', 'thousand', 'million', 'billion', 'trillion', 'quadrillion', 'quintillion', 'sextillion', 'septillion', 'octillion',
           'nonillion', 'decillion')
_ORDINALS = {'one': 'first', 'two': 'second', 'three': 'third', 'five': 'fifth', 'eight': 'eighth', 'nine': 'ninth', 'twelve': 'twelfth'}


def _below_hundred(n):
    return _UNITS[n] if n < 20 else _TENS[n // 10] + ('-' + _UNITS[n % 10] if n % 10 else '')


def number_to_words(num, andword=''):
    ''' the cardinal as the `inflect` package words it: groups of three digits joined by ", ", "thirty-four" hyphenated, `andword`
        in front of the tens and units of a group behind its hundreds and of the last group behind higher groups ("one hundred
        and one", "one thousand and one"); '' leaves it out.  Past 10^36 - 1 the digits are read one by one. '''
    num = int(num)
    if num == 0:
        return 'zero'
    if num >= 10 ** (3 * len(_SCALES)):
        return ' '.join(_UNITS[int(d)] for d in str(num))
    groups, scale = [], 0
    while num:
        num, g = divmod(num, 1000)
        if g:
            words = []
            if g >= 100:
                words.append(_UNITS[g // 100] + ' hundred')
            if g % 100:
                if andword and (g >= 100 or (scale == 0 and num)):
                    words.append(andword)
                words.append(_below_hundred(g % 100))
            groups.append((' '.join(words) + ' ' + _SCALES[scale]).strip())
        scale += 1
    groups.reverse()
    if andword and len(groups) > 1 and groups[-1].startswith(andword + ' '):      # "one thousand and one": no comma in front of "and"
        return ', '.join(groups[:-1]) + ' ' + groups[-1]
    return ', '.join(groups)


def ordinal_to_words(num):
    ''' "2" -> "second", "21" -> "twenty-first", "101" -> "one hundred and first" (`inflect` words ordinals with "and") '''
    words = number_to_words(num, andword='and')
    head, sep, last = words.rpartition('-') if '-' in words.rsplit(' ', 1)[-1] else words.rpartition(' ')
    last = _ORDINALS.get(last) or (last[:-1] + 'ieth' if last.endswith('y') else last + 'th')
    return head + sep + last


def read_integer(n):
    ''' a whole number as it is read aloud: above 1000 and below 3000 as a year -- the century and the rest as two numbers
        ("nineteen ninety-nine", "nineteen oh five"), a full century as "eighteen hundred", the first decade of this millennium as
        "two thousand five" -- and as a cardinal everywhere else '''
    if not 1000 < n < 3000:
        return number_to_words(n)
    century, rest = divmod(n, 100)
    if rest == 0:
        return 'two thousand' if century == 20 else f'{number_to_words(century)} hundred'
    if century == 20 and rest < 10:
        return f'two thousand {_UNITS[rest]}'
    return f'{_below_hundred(century)} {"oh " + _UNITS[rest] if rest < 10 else _below_hundred(rest)}'


def _counted(n, unit):
    return f'{read_integer(n)} {unit}' + ('' if n == 1 else 's')


def _read_amount(match):
    ''' one numeric token of `_NUMERIC`: a pound or dollar amount, or a number with an optional fraction and ordinal ending '''
    if match['pounds'] is not None:
        return _counted(int(match['pounds'].replace(',', '')), 'pound')
    if match['dollars'] is not None:
        pieces = match['dollars'].replace(',', '').split('.')
        if len(pieces) > 2:                                       # not an amount of money: the numbers as they stand
            return ' point '.join(read_integer(int(p)) if p else '' for p in pieces).strip() + ' dollars'
        whole, cents = (int(p) if p else 0 for p in (pieces + [''])[:2])
        said = [_counted(n, unit) for n, unit in ((whole, 'dollar'), (cents, 'cent')) if n]
        return ', '.join(said) if said else 'zero dollars'
    pieces = [match['whole'].replace(',', '')] + (match['fraction'] or '').split('.')[1:]
    said = [read_integer(int(p)) for p in pieces]
    if match['ordinal']:
        said[-1] = ordinal_to_words(pieces[-1])
    return ' point '.join(said)


_NUMERIC = re.compile(r'£(?P<pounds>[\d,]*\d)'                                 # whole pounds
                      r'|\$(?P<dollars>[\d.,]*\d)'                              # dollars, and cents behind a point
                      r'|(?P<whole>\d(?:[\d,]*\d)?)(?P<fraction>(?:\.\d+)+)?(?P<ordinal>st|nd|rd|th)?')


def normalize_numbers(text):
    ''' every number of the text in words, after the rules of the reference's `normalize_numbers.py`: commas inside a number
        only group its digits ("1,000"); "£2" is "two pounds"; "$3.50" is "three dollars, fifty cents" (singular for 1, only the
        part that is not zero, "zero dollars" for none); a decimal point is read "point" and the digits behind it as a number;
        "2nd" is an ordinal; every whole number is read by `read_integer` (years between 1000 and 3000).  One scan over the text
        finds the numeric tokens and `_read_amount` words each.
        A RESTATEMENT that the reference cannot pin on this image: its wording of numbers comes from the `inflect` package, which
        is not installed, so `number_to_words` / `ordinal_to_words` are written from that package's documented behaviour. '''
    return _NUMERIC.sub(_read_amount, text)


# ---- the cleaner (cleaners.py) -----------------------------------------------------------------------------------------------------------

ABBREVIATIONS = {'mrs': 'misess', 'mr': 'mister', 'dr': 'doctor', 'st': 'saint', 'co': 'company', 'jr': 'junior', 'maj': 'major',
                 'gen': 'general', 'drs': 'doctors', 'rev': 'reverend', 'lt': 'lieutenant', 'hon': 'honorable', 'sgt': 'sergeant',
                 'capt': 'captain', 'esq': 'esquire', 'ltd': 'limited', 'col': 'colonel', 'ft': 'fort'}     # (the reference's pairs: data)
# one pass per abbreviation, in the table's order; the dot is part of the abbreviation.  (One pass over all of them at once would
# differ where two abut, "mr.co.": the word boundary in front of the second is gone once the first is spelled out.)
_ABBREVIATION_STAGES = tuple((re.compile(rf'\b{short}[.]', re.IGNORECASE), full) for short, full in ABBREVIATIONS.items())
_TYPOGRAPHIC = {'‘': "'", '’': "'", '“': '"', '”': '"', '–': '-', '—': '--', '…': '...'}
_MARK_RANK = '.!?'                                                                         # of a run of marks the strongest stays


def convert_to_ascii(text):
    ''' the typographic quotes, dashes and the ellipsis as their ASCII spellings, then Unicode NFKD with everything outside ASCII
        dropped ("café" -> "cafe").
        A RESTATEMENT that the reference cannot pin on this image: the reference calls the `unidecode` package, which is not
        installed; `unidecode` also transliterates scripts (Greek, Cyrillic, ...) that are simply dropped here.  One deliberate
        DIFFERENCE from the reference: the pound sign is kept, so that `normalize_numbers` reads "£2" as "two pounds"; `unidecode`
        spells it "PS", so in the reference the pounds rule never sees one behind the fold. '''
    text = ''.join(_TYPOGRAPHIC.get(c, c) for c in text)
    return ''.join(c if c == '£' else unicodedata.normalize('NFKD', c).encode('ascii', 'ignore').decode('ascii') for c in text)


def collapse_whitespace(text):
    return re.sub(r'\s+', ' ', text)


def _strongest_mark(match):
    return max((c for c in match.group(0) if c in _MARK_RANK), key=_MARK_RANK.index) + ' '


# the punctuation stages of the English cleaner, applied in order: a character table (None deletes) or (pattern, replacement)
_PUNCTUATION_STAGES = (
    (re.compile(r' -- '), ', '),                                  # a spaced double dash is a pause ...
    str.maketrans({'-': ' ', '"': None, ';': ',', ':': ','}),     # ... any other hyphen joins two words; quotes go; ; and : pause
    (re.compile(r'[\s.]*[.][\s.]*'), '. '),                       # a run of dots (an ellipsis) and the blanks around it: one full stop
    str.maketrans({'(': None, ')': None}),
    (re.compile(r'[\s,]*,[\s,]*'), ', '),                         # a run of commas and blanks: one comma
    (re.compile(r'[\s_]+'), ' '),                                 # underscores and any white space: one blank
    (re.compile(r'^[ ,.!?-]+'), ''),                              # nothing but a word may open the sentence
    (re.compile(r'[\s.,!?]*[.!?][\s.,!?]*'), _strongest_mark),    # a run of closing marks: the strongest of them (? over ! over .)
)


def english_cleaners(text):
    ''' the reference's English pipeline (`cleaners.py`): ASCII and lower case, numbers and abbreviations in words, then the
        punctuation brought down to single `, . ! ?` marks each followed by one blank.  The stages are those of the reference in
        its order; the three that only ever saw typographic characters are gone, because `convert_to_ascii` has spelled those
        in ASCII by then, and the three passes over closing marks are one (a maximal run holding a ? can hold no other run). '''
    text = normalize_numbers(convert_to_ascii(text).lower())
    for stage in _ABBREVIATION_STAGES + _PUNCTUATION_STAGES:
        text = text.translate(stage) if isinstance(stage, dict) else stage[0].sub(stage[1], text)
    return text.strip()


def text_cleaner(text, lang='english'):
    ''' `cleaners.text_cleaner`: the English pipeline for 'english', the text unchanged for any other language.  Two of its steps
        are restatements that the reference cannot pin on this image (`convert_to_ascii`, `normalize_numbers`: their packages are
        not installed); the rest is pinned by what the reference recorded (tests/golden/text_frontend.json). '''
    return english_cleaners(text) if lang.lower() == 'english' else text


# ---- sentences ---------------------------------------------------------------------------------------------------------------------------

def split_sentence(sentence, language='english'):
    ''' the cleaned sentence as the reference splits it (`generate.py:46-64`), by the tokeniser the feature extraction already
        has (`extract_features.sentence_tokens`): lower-cased words and punctuation marks, the marks in front of the first word
        dropped, of the marks behind the last word the first one kept.  Unlike the reference, which appends None (and then fails)
        when the sentence does not end in a mark, nothing is appended then. '''
    from daft_exprt.extract_features import sentence_tokens
    if language != 'english':
        raise NotImplementedError(f'split_sentence: no character set for language "{language}"')
    tokens, closing = sentence_tokens(text_cleaner(sentence.strip(), language))
    if not tokens:
        raise ValueError(f'no word in "{sentence}"')
    return tokens + ([closing] if closing is not None else [])


def _lookup(sentences_words, dictionary, g2p):
    ''' the phones of every word token of every sentence: from the dictionary, the rest from ONE g2p call over all sentences '''
    tokens = {w for words in sentences_words for w in words if w not in punctuation}
    oov = sorted(w for w in tokens if w not in dictionary)
    found = {}
    if oov:
        decodes = g2p.phonemize(oov) if g2p is not None else [None] * len(oov)
        failed = [w for w, d in zip(oov, decodes) if not d]
        if failed:
            raise ValueError(('no g2p model was given for' if g2p is None else 'the g2p model gives no phones for')
                             + f' the words missing from the dictionary: {", ".join(failed)}')
        found = dict(zip(oov, decodes))
    return found


def _assemble(words, dictionary, found, rng):
    ''' `generate.py:66-82`: words as lists of phones, a punctuation mark or the whitespace symbol between two words, a final eos '''
    words, out = list(words), []
    while words:
        word = words.pop(0)
        if word in dictionary:
            prons = dictionary[word]
            out.append(list(rng.choice(prons) if rng is not None else prons[0]))
        else:
            out.append(list(found[word]))
        if words:
            out.append(words.pop(0) if words[0] in punctuation else whitespace)
    out.append(eos)
    return out


def _dictionary_of(dictionary, hparams):
    if dictionary is None:
        dictionary = hparams.mfa_dictionary
    return dictionary if isinstance(dictionary, dict) else load_dictionary(dictionary, hparams.symbols)


def phonemize_sentences(sentences, hparams, dictionary=None, g2p=None, rng=None, report=None):
    ''' `phonemize_sentence` for a list of sentences with ONE g2p call for the out-of-dictionary words of all of them.  `report`: a
        dict that receives 'oov': {word: phones} for those words, and 'dictionary_words': the word tokens found in the dictionary. '''
    dictionary = _dictionary_of(dictionary, hparams)
    split = [split_sentence(s, hparams.language) for s in sentences]
    found = _lookup(split, dictionary, g2p)
    if report is not None:
        report['oov'] = dict(found)
        report['dictionary_words'] = sum(w in dictionary for words in split for w in words if w not in punctuation)
    return [_assemble(words, dictionary, found, rng) for words in split]


def phonemize_sentence(sentence, hparams, dictionary=None, g2p=None, rng=None):
    ''' `generate.phonemize_sentence` (`generate.py:28-107`), step by step: the sentence is cleaned (`text_cleaner`), lower-cased and
        split into words and punctuation marks (`split_sentence`); every word becomes the list of its phones, two words are
        separated by the punctuation mark between them or else by the whitespace symbol, and the list ends with the eos symbol.
        "that's, an 'example! ' of a sentence. '" -> [that's] , [an] ' ' [example'] ! [of] ' ' [a] ' ' [sentence] . ~
          dictionary  `{word: [phones, ...]}` (`load_dictionary`) or a path; None: `hparams.mfa_dictionary`
          g2p         a `g2p.G2P` for the words the dictionary lacks: all of them go to it in one batch.  The reference writes them
                      to a file and runs `mfa g2p` on it (84-105)
          rng         with several pronunciations the FIRST listed is taken, unless `rng` (a `random.Random`, or the `random`
                      module) is given, whose `choice` then draws one -- the reference always draws with `random.choice`
        A word missing from the dictionary with g2p=None, or for which the g2p gives nothing, raises ValueError listing the words: no
        word is dropped, and `<unk>` is never emitted. '''
    return phonemize_sentences([sentence], hparams, dictionary, g2p, rng)[0]


def format_sentence(sentence):
    ''' one phonemised sentence as `sentences_to_generate.txt` holds it (`generate.py:486-491`): `{P1 P2} , {P3} ? ~` '''
    text = ''
    for item in sentence:
        if isinstance(item, (list, tuple)):
            item = '{' + ' '.join(item) + '}'
        text = f'{text} {item} '
    return collapse_whitespace(text).strip()


def prepare_sentences_for_inference(text_file, output_dir, hparams, g2p=None, dictionary=None, rng=None, report=None):
    ''' `generate.prepare_sentences_for_inference` (`generate.py:465-494`): phonemises the lines of `text_file` and writes
        `<output_dir>/sentences_to_generate.txt`, one `file_name|{P1 P2} {P3} , {P4} ? ~` per line -- exactly what
        `generate.read_phonemised_sentences` reads back.  Returns (sentences, file_names).  A line is named
        `<basename of text_file>_line<idx>` as in the reference; a line of the form `name|text` is named `name` instead, so the
        transcripts of a corpus can be phonemised under their own names.  Empty lines are skipped (their index is not reused).
        Differences from the reference: `output_dir` is created when missing but NOT deleted when it exists; the words missing from
        the dictionary are phonemised together for ALL sentences (one g2p batch) instead of once per sentence; there is no
        `n_jobs`.  dictionary, rng, report: as `phonemize_sentences`. '''
    if not os.path.isfile(text_file):
        raise FileNotFoundError(f'There is no such file {text_file}')
    with open(text_file, 'r', encoding='utf-8') as f:
        lines = [line.strip() for line in f]
    texts, file_names = [], []
    for idx, line in enumerate(lines):
        if not line:
            continue
        name, bar, text = line.partition('|')
        named = bool(bar) and bool(name.strip()) and not re.search(r'\s', name.strip())
        texts.append(text if named else line)
        file_names.append(name.strip() if named else f'{os.path.basename(text_file)}_line{idx}')
    sentences = phonemize_sentences(texts, hparams, dictionary, g2p, rng, report)
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, 'sentences_to_generate.txt'), 'w', encoding='utf-8') as f:
        for sentence, file_name in zip(sentences, file_names):
            f.write(f'{file_name}|{format_sentence(sentence)}\n')
    return sentences, file_names
