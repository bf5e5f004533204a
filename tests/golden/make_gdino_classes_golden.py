"""Generate tests/golden/gdino_classes_small.npz: the REFERENCE's own closed-set helpers (GD/util/vl_utils.py:
build_captions_and_token_span, create_positive_map_from_span) run with HuggingFace's BertTokenizerFast over the toy
vocabulary of tests/test_caption_cpu.py (build container only: needs `transformers` and the reference checkout; nothing
is written into /root/reference, and vl_utils.py is loaded by path, without the package around it).

Stored, per case: the caption, the character spans, the tokenizer's input ids and offset mapping, and the positive map
[n, 256] exactly as create_positive_map_from_span returned it.  Cases:
  classes_*   class lists through build_captions_and_token_span (a two-word class, a one-letter class, an accented
              class, a class that splits into several pieces, an unknown word) - no name contains "/", where the
              reference would draw a random alternative
  spans       a free caption with hand-set spans: a span that ends on a blank and one that begins on one (the +1/+2 and
              -2/-3 retries), a span inside a run of blanks (no token: a zero row), a span over "##" pieces, two spans
              for one phrase
"""
import importlib.util
import json
import tempfile
from pathlib import Path

import numpy as np

VL_UTILS = "/root/reference/InkLayer/third_party/GroundingDINO/groundingdino/util/vl_utils.py"
TOY = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", ".", ",", "'", "?", "!", "cat", "dog", "tea", "##pot", "##s", "cafe", "a",
       "s", "don", "t", "n't", "is", "it", "'s", "sit", "##ting", "猫"]

CLASS_LISTS = {
    "classes_basic": ["cat", "tea pots", "a", "Café", "dog"],
    "classes_pieces": ["teapots", "sitting cat", "zebra", "dog"],
    "classes_one": ["s"],
}
#                     0123456789012345678901234567890123
SPAN_CAPTION = "cat      teapots, café sitting dog"          # preprocess_caption adds the "."
SPAN_CASES = [
    [[0, 4]],               # "cat " - ends on a blank: end - 2
    [[8, 16]],              # " teapots" - begins on a blank: beg + 1
    [[4, 7]],               # blanks only: no token, a zero row
    [[9, 16]],              # tea ##pot ##s
    [[18, 22], [31, 34]],   # café + dog: two spans of one phrase
    [[23, 30]],             # sit ##ting
    [[12, 14]],             # inside "teapots": the pieces that hold characters 12 and 13
]


def main():
    from transformers import BertTokenizerFast
    spec = importlib.util.spec_from_file_location("ref_vl_utils", VL_UTILS)
    vl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vl)
    with tempfile.TemporaryDirectory() as d:
        vocab = Path(d) / "vocab.txt"
        vocab.write_text("\n".join(TOY) + "\n", encoding="utf-8")
        tok = BertTokenizerFast(str(vocab), do_lower_case=True)
    out = {"vocab": np.array(json.dumps(TOY))}
    for name, classes in CLASS_LISTS.items():
        caption, cat2span = vl.build_captions_and_token_span(classes, True)
        spans = [cat2span[c.lower()] for c in classes]
        enc = tok(caption, return_offsets_mapping=True)
        pm = vl.create_positive_map_from_span(tok(caption), spans)
        out[name] = np.array(json.dumps(dict(classes=classes, caption=caption, spans=spans, ids=enc["input_ids"],
                                             offsets=[list(o) for o in enc["offset_mapping"]])))
        out[name + "_map"] = pm.numpy()
    caption = SPAN_CAPTION.lower().strip()
    caption = caption if caption.endswith(".") else caption + "."      # inference_on_a_image.py:86-89
    enc = tok(caption, return_offsets_mapping=True)
    pm = vl.create_positive_map_from_span(tok(caption), SPAN_CASES)
    out["spans"] = np.array(json.dumps(dict(caption_in=SPAN_CAPTION, caption=caption, spans=SPAN_CASES,
                                            ids=enc["input_ids"], offsets=[list(o) for o in enc["offset_mapping"]])))
    out["spans_map"] = pm.numpy()
    path = Path(__file__).with_name("gdino_classes_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, path.stat().st_size, "bytes")
    for k, v in out.items():
        if not k.endswith("_map") and k != "vocab":
            print(k, json.loads(str(v)))
        elif k.endswith("_map"):
            print(k, [np.nonzero(r)[0].tolist() for r in v])


if __name__ == "__main__":
    main()
