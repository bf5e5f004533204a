"""Host side of closed-set detection: a class list becomes ONE caption, character spans and a normalised positive map,
as the reference's evaluation does it (GD/util/vl_utils.py:8-87, used by PostProcessCocoGrounding,
GD/demo/test_ap_on_coco.py:66-88, and by the given-phrase mode of GD/demo/inference_on_a_image.py:117-122).

    caption, spans = build_captions_and_token_span(["cat", "hot dog"])      # "cat . hot dog ."
    ids, offsets = tokenizer.encode_with_offsets(caption, preprocess=False)
    pm = positive_map_from_spans(offsets, spans)                            # f32 [2, 256], rows sum to n / (n + 1e-6)

`class_prompt` does the three steps and refuses a class list whose caption does not fit.  The scores themselves are the
engine's: GDinoEngine.predict_classes / predict_spans on ops.class_scores (csrc/closed_set.hip).

Where this differs from the reference, on purpose:
  - a class name that contains "/" is taken AS WRITTEN.  vl_utils.py:66-69 picks one of its alternatives (or the whole
    name) with random.choice, so the caption - and with it every score - changes from call to call; a detector like
    that can be neither tested nor cached.  Name the alternative you want.
  - build_captions_and_token_span returns the spans as a LIST in class order, not a dict keyed by the (lower-cased)
    name: a dict drops a repeated name and cannot be indexed by the name as given.  A name without a word (empty,
    blanks only) has no span, adds nothing to the caption and scores exactly 0 for every box.
  - no SHILONG_DEBUG_ONLY_ONE_POS switch.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from .wordpiece import char_to_token

Span = Tuple[int, int]


def build_captions_and_token_span(class_names: Sequence[str], force_lowercase: bool = True) -> Tuple[str, List[List[Span]]]:
    """vl_utils.py:49-87: the words of every class joined by single spaces, " ." after each class; one half-open
    character span per word.  -> (caption, spans[class] = [(start, end), ...])."""
    caption, spans = "", []
    for name in class_names:
        name = name.lower() if force_lowercase else name
        mine: List[Span] = []
        for word in (w.strip() for w in name.strip().split(" ")):
            if not word:
                continue
            if caption:
                caption += " "
            mine.append((len(caption), len(caption) + len(word)))
            caption += word
        if mine:
            caption += " ."
        spans.append(mine)
    return caption, spans


def positive_map_from_spans(offsets: Sequence[Span], token_spans: Sequence[Sequence[Span]],
                            max_text_len: int = 256) -> torch.Tensor:
    """create_positive_map_from_span (vl_utils.py:8-46) over WordPiece.encode_with_offsets' offsets: row j is 1 on the
    tokens from the one that holds a span's first character to the one that holds its last, for every span of class /
    phrase j, then divided by (its sum + 1e-6).  A span whose first character is not in a token (a blank) is tried one
    and two characters later, one whose last is not, one and two earlier, as the reference does; a span that still finds
    no token is skipped.  -> f32 [len(token_spans), max_text_len]."""
    pm = torch.zeros((len(token_spans), max_text_len), dtype=torch.float32)
    for j, spans in enumerate(token_spans):
        for beg, end in spans:
            beg_pos, end_pos = char_to_token(offsets, beg), char_to_token(offsets, end - 1)
            if beg_pos is None:
                beg_pos = char_to_token(offsets, beg + 1)
                if beg_pos is None:
                    beg_pos = char_to_token(offsets, beg + 2)
            if end_pos is None:
                end_pos = char_to_token(offsets, end - 2)
                if end_pos is None:
                    end_pos = char_to_token(offsets, end - 3)
            if beg_pos is None or end_pos is None:
                continue
            pm[j, beg_pos:end_pos + 1] = 1.0
    return pm / (pm.sum(-1)[:, None] + 1e-6)


class ClassPrompt(NamedTuple):
    """A class list (or a caption with phrase spans) ready for the engine."""
    token_ids: Tuple[int, ...]        # [CLS] ... [SEP] of the caption
    positive_map: torch.Tensor        # f32 [C, max_text_len]
    caption: Optional[str]
    names: Tuple[str, ...]            # the classes as given (labels index this)


def class_prompt(tokenizer, class_names: Sequence[str], max_text_len: int = 256,
                 force_lowercase: bool = True) -> ClassPrompt:
    """Caption, token ids and positive map of a class list.  ValueError for an empty list and for one whose caption has
    more than max_text_len tokens - cutting it would silently drop the last classes; the message says how many fit."""
    names = tuple(class_names)
    if not names:
        raise ValueError("closed-set detection needs at least one class")
    caption, spans = build_captions_and_token_span(names, force_lowercase)
    ids, offsets = tokenizer.encode_with_offsets(caption, preprocess=False)
    if len(ids) > max_text_len:
        fit, used = 0, 2                                # [CLS] and [SEP]
        for name, sp in zip(names, spans):
            used += sum(len(tokenizer.tokenize(caption[s:e])) for s, e in sp) + (1 if sp else 0)
            if used > max_text_len:
                break
            fit += 1
        raise ValueError(f"the caption of these {len(names)} classes has {len(ids)} tokens, the detector takes "
                         f"{max_text_len}: only the first {fit} classes fit - split the list and merge the results")
    return ClassPrompt(tuple(ids), positive_map_from_spans(offsets, spans, max_text_len), caption, names)


def span_prompt(tokenizer, caption: str, token_spans: Sequence[Sequence[Span]], max_text_len: int = 256) -> ClassPrompt:
    """The given-phrase mode (inference_on_a_image.py:86-89, 119-122): the caption goes through preprocess_caption, the
    spans are character positions in THAT string, one list of spans per phrase."""
    ids, offsets = tokenizer.encode_with_offsets(caption, preprocess=True)
    if len(ids) > max_text_len:
        raise ValueError(f"the caption has {len(ids)} tokens, the detector takes {max_text_len}")
    from .wordpiece import preprocess_caption
    text = preprocess_caption(caption)
    names = tuple(" ".join(text[s:e] for s, e in sp) for sp in token_spans)
    return ClassPrompt(tuple(ids), positive_map_from_spans(offsets, token_spans, max_text_len), text, names)
