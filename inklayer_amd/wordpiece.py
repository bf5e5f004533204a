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
"""
from __future__ import annotations

import os
import unicodedata
from typing import Dict, List, Optional, Sequence

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

    def decode(self, ids: Sequence[int]) -> str:
        """Tokens joined by spaces, "##" pieces merged, then clean_up_tokenization's replacements."""
        text = " ".join(self.tokens[int(i)] for i in ids).replace(" ##", "")
        for a, b in ((" .", "."), (" ?", "?"), (" !", "!"), (" ,", ","), (" ' ", "'"), (" n't", "n't"), (" 'm", "'m"),
                     (" 's", "'s"), (" 've", "'ve"), (" 're", "'re")):
            text = text.replace(a, b)
        return text
