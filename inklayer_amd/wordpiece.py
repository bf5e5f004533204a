"""A small BERT-uncased WordPiece tokenizer over a user-supplied vocab.txt, for GroundingDINO captions.

Restates what the reference's tokenizer (AutoTokenizer "bert-base-uncased" -> BertTokenizer: BasicTokenizer with
do_lower_case + WordpieceTokenizer, and decode's clean_up_tokenization) does to a caption: lower-casing, NFD accent
stripping, whitespace and punctuation splitting, control-character removal, spaces around CJK ideographs, greedy
longest-match WordPiece with "##" continuation pieces, [UNK] for a word without a match or over 100 characters,
[CLS] ... [SEP].

Parity with HuggingFace is UNPINNED OFFLINE: the bert-base-uncased vocabulary is not available where this was written
and the installed `transformers` does not build a usable BertTokenizer from a bare vocab file, so the tests check
hand-worked expectations on a toy vocabulary, not HuggingFace's output.  The token ids are DATA (see text_branch.py):
without a vocabulary every detector API still takes id lists, and phrases come back as id tuples.
One exception: BertTokenizerFast (the `tokenizers` library) does load the toy vocabulary, and the ids and character
offsets of the captions in tests/golden/gdino_classes_small.npz are its output (encode_with_offsets is compared with
them exactly, tests/test_closed_set_cpu.py).
"""
from __future__ import annotations

import os
import unicodedata
from typing import Dict, List, Optional, Sequence, Tuple

MAX_CHARS_PER_WORD = 100


def preprocess_caption(caption: str) -> str:
    """GD/util/inference.py:22-26: lower, strip, a trailing "." """
    result = caption.lower().strip()
    return result if result.endswith(".") else result + "."


def default_vocab_path() -> Optional[str]:
    """models/bert-base-uncased/vocab.txt (InkLayer.utils.paths.get_model_path) if it exists, else $INKLAYER_BERT_VOCAB."""
    try:
        from InkLayer.utils.paths import get_model_path
        p = get_model_path("bert-base-uncased/vocab.txt")
        if p and os.path.isfile(p):
            return p
    except ImportError:
        pass
    p = os.environ.get("INKLAYER_BERT_VOCAB")
    return p if p and os.path.isfile(p) else None


def _is_whitespace(ch: str) -> bool:
    return ch in " \t\n\r" or unicodedata.category(ch) == "Zs"


def _is_control(ch: str) -> bool:
    if ch in "\t\n\r":
        return False
    return unicodedata.category(ch).startswith("C")


def _is_punctuation(ch: str) -> bool:
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:     # all non-alphanumeric ASCII
        return True
    return unicodedata.category(ch).startswith("P")


def _is_cjk(cp: int) -> bool:
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F
            or 0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF
            or 0x2F800 <= cp <= 0x2FA1F)


def basic_tokenize(text: str) -> List[str]:
    """BasicTokenizer(do_lower_case=True): clean, space CJK, split on whitespace, lower, strip accents, split
    punctuation."""
    cleaned = []
    for ch in text:
        cp = ord(ch)
        if cp == 0 or cp == 0xFFFD or _is_control(ch):
            continue
        if _is_cjk(cp):
            cleaned += [" ", ch, " "]
        else:
            cleaned.append(" " if _is_whitespace(ch) else ch)
    out: List[str] = []
    for word in "".join(cleaned).split():
        word = unicodedata.normalize("NFD", word.lower())
        word = "".join(ch for ch in word if unicodedata.category(ch) != "Mn")
        cur = ""
        for ch in word:
            if _is_punctuation(ch):
                if cur:
                    out.append(cur)
                out.append(ch)
                cur = ""
            else:
                cur += ch
        if cur:
            out.append(cur)
    return out


def basic_tokenize_with_offsets(text: str) -> List[Tuple[str, List[int]]]:
    """basic_tokenize, with every character of a token carrying the index in `text` of the character it came from:
    [(token, [index per character])].  Lower-casing and accent stripping are done per original character (a stripped
    accent leaves its base character's index; a character whose lower-case form is several characters gives them all
    its index), so the indices always point into `text` as it was given."""
    words: List[List[int]] = []
    cur: List[int] = []
    for i, ch in enumerate(text):
        cp = ord(ch)
        if cp == 0 or cp == 0xFFFD or _is_control(ch):
            continue                                   # removed without ending a word, as basic_tokenize's clean-up
        if _is_cjk(cp) or _is_whitespace(ch) or ch.isspace():      # (str.split's own idea of a space included)
            if cur:
                words.append(cur)
            cur = []
            if _is_cjk(cp):
                words.append([i])
        else:
            cur.append(i)
    if cur:
        words.append(cur)
    out: List[Tuple[str, List[int]]] = []
    for idxs in words:
        lowered = "".join(text[i] for i in idxs).lower()      # of the WORD: str.lower looks at context (final sigma)
        chars: List[Tuple[str, int]] = []
        for i in idxs:
            chars += [(c, i) for c in text[i].lower()]
        if len(lowered) == len(chars):
            chars = [(c, i) for c, (_, i) in zip(lowered, chars)]
        norm = [(c, i) for ch, i in chars for c in unicodedata.normalize("NFD", ch) if unicodedata.category(c) != "Mn"]
        tok, where = "", []
        for c, i in norm:
            if _is_punctuation(c):
                if tok:
                    out.append((tok, where))
                out.append((c, [i]))
                tok, where = "", []
            else:
                tok += c
                where.append(i)
        if tok:
            out.append((tok, where))
    return out


def char_to_token(offsets: Sequence[Tuple[int, int]], i: int) -> Optional[int]:
    """BatchEncoding.char_to_token over WordPiece.encode_with_offsets' offsets: the index of the token whose half-open
    span contains character i; None for whitespace or a position outside the caption ([CLS] / [SEP] span nothing)."""
    for k, (s, e) in enumerate(offsets):
        if s <= i < e:
            return k
    return None


class WordPiece:
    """tokenizer(caption) -> ids and decode(ids) -> str over one vocab.txt (one token per line, the line number its id)."""

    def __init__(self, vocab_path: Optional[str] = None):
        vocab_path = vocab_path or default_vocab_path()
        if vocab_path is None:
            raise FileNotFoundError("no BERT vocabulary: pass the path of bert-base-uncased's vocab.txt, put it at "
                                    "models/bert-base-uncased/vocab.txt, or set INKLAYER_BERT_VOCAB")
        with open(vocab_path, "r", encoding="utf-8") as f:
            self.tokens: List[str] = [line.rstrip("\n") for line in f]
        self.vocab: Dict[str, int] = {t: i for i, t in enumerate(self.tokens)}
        for special in ("[UNK]", "[CLS]", "[SEP]"):
            if special not in self.vocab:
                raise ValueError(f"{vocab_path} is not a BERT vocabulary: {special} is missing")
        self.unk, self.cls, self.sep = (self.vocab[t] for t in ("[UNK]", "[CLS]", "[SEP]"))

    def wordpiece(self, word: str) -> List[str]:
        """Greedy longest-match-first pieces of one basic token; ["[UNK]"] when a piece has no match."""
        if len(word) > MAX_CHARS_PER_WORD:
            return ["[UNK]"]
        pieces, start = [], 0
        while start < len(word):
            end, cur = len(word), None
            while start < end:
                sub = ("##" if start else "") + word[start:end]
                if sub in self.vocab:
                    cur = sub
                    break
                end -= 1
            if cur is None:
                return ["[UNK]"]
            pieces.append(cur)
            start = end
        return pieces

    def tokenize(self, text: str) -> List[str]:
        return [p for w in basic_tokenize(text) for p in self.wordpiece(w)]

    def encode(self, caption: str, preprocess: bool = True) -> List[int]:
        """[CLS] pieces [SEP] of the caption (preprocess_caption first, as predict does)."""
        text = preprocess_caption(caption) if preprocess else caption
        return [self.cls] + [self.vocab[p] for p in self.tokenize(text)] + [self.sep]

    __call__ = encode

    def encode_with_offsets(self, caption: str, preprocess: bool = True) -> Tuple[List[int], List[Tuple[int, int]]]:
        """encode's ids, and for each the half-open character span (start, end) it covers in the string that was
        tokenized - preprocess_caption(caption) with preprocess, the caption itself without - as a fast tokenizer's
        offset mapping gives them: [CLS] and [SEP] get (0, 0), a "##" piece the characters it continues with, an [UNK]
        its whole word.  Lower-casing and accent stripping leave the spans on the ORIGINAL characters."""
        text = preprocess_caption(caption) if preprocess else caption
        ids, offsets = [self.cls], [(0, 0)]
        for word, where in basic_tokenize_with_offsets(text):
            pieces = self.wordpiece(word)
            if pieces == ["[UNK]"]:
                ids.append(self.unk)
                offsets.append((where[0], where[-1] + 1))
                continue
            at = 0
            for p in pieces:
                n = len(p) - 2 if at else len(p)       # a continuation piece carries "##"
                ids.append(self.vocab[p])
                offsets.append((where[at], where[at + n - 1] + 1))
                at += n
        return ids + [self.sep], offsets + [(0, 0)]

    def decode(self, ids: Sequence[int]) -> str:
        """Tokens joined by spaces, "##" pieces merged, then clean_up_tokenization's replacements."""
        text = " ".join(self.tokens[int(i)] for i in ids).replace(" ##", "")
        for a, b in ((" .", "."), (" ?", "?"), (" !", "!"), (" ,", ","), (" ' ", "'"), (" n't", "n't"), (" 'm", "'m"),
                     (" 's", "'s"), (" 've", "'ve"), (" 're", "'re")):
            text = text.replace(a, b)
        return text
