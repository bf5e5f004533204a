"""Detector plugin (reference: InkLayer/detector/gdino.py:12-30), MI355X engine underneath.

`run_ft_dino_on_sketch(path) -> {"bboxes": normalised xyxy lists, "scores": [...], "labels": [...]}`
with caption "object", box_threshold 0.2, text_threshold 0 exactly as the reference.  The model is a
module-level singleton like the reference's `model`, but created on first use and kept resident in
HBM (the reference re-`.to(device)`s it every call, GD/util/inference.py:64).

`predict(model, image, caption, box_threshold, text_threshold)` is the reference's open-vocabulary call
(GD/util/inference.py:54-97): any caption of up to 256 tokens, a phrase per box.  `run_gdino_on_sketch` wraps it in
run_ft_dino_on_sketch's dict shape with the real labels.  `predict_batch` / `run_gdino_on_sketches` take a batch of
images with one caption each and run it as one forward (per-image token counts and text padding masks).

Closed-set detection - a class index per box, scored as the reference's evaluation does (PostProcessCocoGrounding,
GD/demo/test_ap_on_coco.py:66-137) with the scores, the selection and the box conversion on the GPU:
`predict_classes(model, image, classes, num_select=300)`, `predict_classes_batch` (one class list per image),
`predict_spans` (the given-phrase mode of GD/demo/inference_on_a_image.py:117-142) and `run_gdino_on_sketch_classes(path,
nouns, score_threshold=0.2)`, the dict of the reference's closed-set detector (InkLayer/detector/gdino_mmdetection.py)."""
import os
import re

import numpy as np
from PIL import Image

from InkLayer.utils.paths import get_model_path
from InkLayer.utils.processing import cxcywh_to_xyxy

gdino_config_path = get_model_path("GroundingDINO_SwinT_OGC.py")
weights_path = get_model_path("inklayer_gdino.pth")
model = None


def backbone_of_config(config_path):
    """The `backbone = "..."` name of a GroundingDINO config file (GroundingDINO_SwinT_OGC.py / GroundingDINO_SwinB_cfg.py),
    read as TEXT - the file is never executed.  None when there is no such file or no such line."""
    if not config_path or not os.path.isfile(config_path):
        return None
    with open(config_path, "r", encoding="utf-8", errors="replace") as f:
        m = re.search(r"""^\s*backbone\s*=\s*["']([A-Za-z0-9_]+)["']""", f.read(), flags=re.M)
    return m.group(1) if m else None


def random_weights_model():
    """The registry name INKLAYER_GDINO_MODEL picks for INKLAYER_RANDOM_WEIGHTS=1 (default swin_t); ValueError for a
    name the registry does not have, before anything is built."""
    from inklayer_amd import gdino
    name = os.environ.get("INKLAYER_GDINO_MODEL", "swin_t")
    gdino.config_for(name)
    return name


def load_model(config_path=None, checkpoint_path=None, device="cuda"):
    """groundingdino.util.inference.load_model (GD/util/inference.py:29-36) for the HIP engine.  The defaults are the
    module attributes `gdino_config_path` / `weights_path`, read at CALL time.  The model (Swin-T or Swin-B, window 7 or
    12, layer counts) is read off the checkpoint's tensor shapes; a config file, where one exists, is only cross-checked:
    its backbone name must be the checkpoint's (ValueError otherwise)."""
    import torch
    checkpoint_path = weights_path if checkpoint_path is None else checkpoint_path
    config_path = gdino_config_path if config_path is None else config_path
    from inklayer_amd import gdino, text_branch, weights_init
    if os.environ.get("INKLAYER_RANDOM_WEIGHTS") == "1":      # no checkpoints exist offline
        cfg = gdino.config_for(random_weights_model())
        sd = weights_init.random_gdino_state_dict(cfg, device)
        text = weights_init.random_text_features(cfg, device)
    else:
        if not os.path.exists(checkpoint_path):
            raise FileNotFoundError(f"Checkpoint not found at {checkpoint_path}")
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        sd = gdino.clean_state_dict(ckpt["model"] if "model" in ckpt else ckpt)   # GD/util/inference.py:33-34
        cfg = gdino.config_from_state_dict(sd)
        named, held = backbone_of_config(config_path), gdino.model_name(cfg)
        if named is not None and named != held:
            raise ValueError(f"{config_path} names backbone {named!r}, but {checkpoint_path} holds "
                             f"{held or 'a Swin backbone outside the registry'} (embed dim {cfg.embed_dim}, depths "
                             f"{cfg.depths}, heads {cfg.num_heads}, window {cfg.window_size}): use the config that "
                             f"belongs to the checkpoint")
        text = text_branch.encode_caption_from_checkpoint(sd, gdino.DEFAULT_TOKEN_IDS)
    eng = gdino.GDinoEngine(sd, cfg, device, encoded_text=text)
    if os.environ.get("INKLAYER_RANDOM_WEIGHTS") != "1":      # later captions fold BERT from the same checkpoint
        eng.text_weights = {k: v for k, v in sd.items() if k.startswith(("bert.", "feat_map."))}
    return eng


def get_model():
    global model
    if model is None:
        model = load_model()
    return model


def run_ft_dino_on_sketch(sketch_path):
    import torch
    from inklayer_amd import gdino
    eng = get_model()
    image_source = np.asarray(Image.open(sketch_path).convert("RGB"))
    from inklayer_amd import ops
    raw = torch.from_numpy(np.ascontiguousarray(image_source)).to(eng.dev)
    oh, ow = gdino.resize_shape(image_source.shape[1], image_source.shape[0])   # load_image's RandomResize([800], 1333)
    boxes, scores = eng.detect([ops.resize_bilinear_u8(raw, oh, ow)])[0]
    normalized = cxcywh_to_xyxy(boxes.tolist()).tolist()        # cxcywh -> xyxy in float64
    return {"bboxes": normalized, "scores": scores.tolist(), "labels": ["object"] * len(normalized)}


_tokenizer = None


def get_tokenizer():
    """The BERT-uncased WordPiece tokenizer over models/bert-base-uncased/vocab.txt or $INKLAYER_BERT_VOCAB
    (FileNotFoundError without one: captions are then given as token ids)."""
    global _tokenizer
    if _tokenizer is None:
        from inklayer_amd.wordpiece import WordPiece
        _tokenizer = WordPiece()
    return _tokenizer


def _caption_ids(caption):
    """(token ids, tokenizer or None) of a caption given as text (needs the vocabulary) or as a sequence of ids."""
    if isinstance(caption, str):
        tok = get_tokenizer()
        return tok.encode(caption), tok
    try:
        tok = get_tokenizer()
    except FileNotFoundError:
        tok = None
    return [int(t) for t in caption], tok


def predict(model, image, caption, box_threshold, text_threshold, device="cuda", remove_combined=False):
    """groundingdino.util.inference.predict (GD/util/inference.py:54-97) on the HIP engine `model` (load_model):
    image an HWC uint8 RGB array or a path (resized as load_image does, on the GPU), caption a str - tokenized with the
    BERT vocabulary - or a sequence of token ids ([CLS] ... [SEP]).  -> (boxes [n, 4] cxcywh normalised, scores [n],
    phrases): phrases are strings where a vocabulary is available and id tuples otherwise.  `device` is accepted for the
    reference's signature; the engine stays where it was loaded.  A caller that keeps one caption over many images sets
    it once with model.set_caption and calls model.predict, which also keeps the captured HIP graphs."""
    import torch
    from inklayer_amd import gdino, ops
    ids, tok = _caption_ids(caption)
    if isinstance(image, (str, os.PathLike)):
        image = np.asarray(Image.open(image).convert("RGB"))
    raw = torch.from_numpy(np.ascontiguousarray(image)).to(model.dev)
    oh, ow = gdino.resize_shape(image.shape[1], image.shape[0])
    # like the reference's, this call is stateless in the caption: the engine (the singleton run_ft_dino_on_sketch
    # shares) leaves with the caption and tokenizer it came with; its features wait in the engine's caption cache
    held_ids, held_tok = tuple(model.token_ids), model.tokenizer
    try:
        if tuple(ids[:model.cfg.max_text_len]) != held_ids:
            text = None
            if os.environ.get("INKLAYER_RANDOM_WEIGHTS") == "1":  # no BERT weights either: stand-in features, as load_model
                from inklayer_amd import weights_init
                text = weights_init.random_text_features(model.cfg, "cpu", n_tokens=min(len(ids), model.cfg.max_text_len))
            model.set_caption(ids, encoded_text=text)
        model.tokenizer = tok
        return model.predict([ops.resize_bilinear_u8(raw, oh, ow)], box_threshold, text_threshold, remove_combined)[0]
    finally:
        if tuple(model.token_ids) != held_ids:
            model.set_caption(held_ids)
        model.tokenizer = held_tok


def predict_batch(model, images, captions, box_threshold, text_threshold, remove_combined=False):
    """predict for a batch with ONE CAPTION PER IMAGE (GroundingDINO.forward with a list of captions): images are HWC
    uint8 RGB arrays or paths, captions strs or sequences of token ids, one per image.  -> [(boxes, scores, phrases)] in
    input order.  One forward for the batch (size groups for images of different sizes) on the engine's per-image form
    (GDinoEngine.set_captions): every image is scored against its own caption only and pays for its own token count.
    Stateless like predict: the engine leaves with the caption(s), features and tokenizer it came with."""
    import torch
    from inklayer_amd import gdino, ops
    images, captions = list(images), list(captions)
    if len(images) != len(captions):
        raise ValueError(f"{len(images)} images for {len(captions)} captions: predict_batch takes one caption per image")
    if not images:
        return []
    tok, id_lists = None, []
    for c in captions:
        ids, tok = _caption_ids(c)
        id_lists.append(ids)
    resized = []
    for image in images:
        if isinstance(image, (str, os.PathLike)):
            image = np.asarray(Image.open(image).convert("RGB"))
        raw = torch.from_numpy(np.ascontiguousarray(image)).to(model.dev)
        oh, ow = gdino.resize_shape(image.shape[1], image.shape[0])
        resized.append(ops.resize_bilinear_u8(raw, oh, ow))
    texts = None
    if os.environ.get("INKLAYER_RANDOM_WEIGHTS") == "1":      # no BERT weights: stand-in features per caption, as predict
        from inklayer_amd import weights_init
        texts = [weights_init.random_text_features(model.cfg, "cpu", n_tokens=min(len(ids), model.cfg.max_text_len))
                 for ids in id_lists]
    # the held state with its features: a batch of many captions may push them out of the engine's caption cache
    held_tok, held_caps, held_ids, held_text = model.tokenizer, model.captions, model.token_ids, model.text0.cpu()
    held_lens, held_tmax = model.t_lens, model.Tmax
    try:
        model.set_captions(id_lists, encoded_texts=texts)
        model.tokenizer = tok
        return model.predict(resized, box_threshold, text_threshold, remove_combined)
    finally:
        if held_caps is None:
            model.set_caption(held_ids, encoded_text=held_text)
        else:
            rows = held_text.view(len(held_caps), held_tmax, 256)
            model.set_captions(held_caps, encoded_texts=[rows[b, :n] for b, n in enumerate(held_lens)])
        model.tokenizer = held_tok


class _held_text:
    """with _held_text(model): ... - the engine leaves with the caption(s), features and tokenizer it came with, in the
    shared and in the per-image form (the features travel along: many captions may push them out of the cache)."""

    def __init__(self, model):
        self.m = model

    def __enter__(self):
        m = self.m
        self.held = (m.tokenizer, m.captions, m.token_ids, m.text0.cpu(), m.t_lens, m.Tmax)
        return m

    def __exit__(self, *exc):
        m = self.m
        tok, caps, ids, text, lens, tmax = self.held
        if caps is None:
            if m.captions is not None or tuple(m.token_ids) != tuple(ids):
                m.set_caption(ids, encoded_text=text)
        else:
            rows = text.view(len(caps), tmax, 256)
            m.set_captions(caps, encoded_texts=[rows[b, :n] for b, n in enumerate(lens)])
        m.tokenizer = tok
        return False


def _class_prompt(model, classes):
    """A closed_set.ClassPrompt as it is, or the prompt of a list of class names (needs the vocabulary, as a caption
    given as text does)."""
    from inklayer_amd import closed_set
    if isinstance(classes, closed_set.ClassPrompt):
        return classes
    if isinstance(classes, str):
        raise TypeError("classes is a list of class names, not one string")
    return closed_set.class_prompt(get_tokenizer(), list(classes), model.cfg.max_text_len)


def _load_resized(model, image):
    """(resized HWC uint8 image on the engine's device, (h, w) of the original) of an array or a path."""
    import torch
    from inklayer_amd import gdino, ops
    if isinstance(image, (str, os.PathLike)):
        image = np.asarray(Image.open(image).convert("RGB"))
    raw = torch.from_numpy(np.ascontiguousarray(image)).to(model.dev)
    oh, ow = gdino.resize_shape(image.shape[1], image.shape[0])
    return ops.resize_bilinear_u8(raw, oh, ow), (int(image.shape[0]), int(image.shape[1]))


def _set_prompts(model, prompts):
    """The engine's caption(s) := the prompts' (stand-in features under INKLAYER_RANDOM_WEIGHTS=1, as predict)."""
    texts = [None] * len(prompts)
    if os.environ.get("INKLAYER_RANDOM_WEIGHTS") == "1":
        from inklayer_amd import weights_init
        texts = [weights_init.random_text_features(model.cfg, "cpu", n_tokens=len(p.token_ids)) for p in prompts]
    if len(prompts) == 1:
        if model.captions is not None or tuple(model.token_ids) != tuple(prompts[0].token_ids):
            model.set_caption(prompts[0].token_ids, encoded_text=texts[0])
    else:
        model.set_captions([p.token_ids for p in prompts], encoded_texts=texts)


def predict_classes_batch(model, images, class_lists, num_select=300, normalized=False):
    """Closed-set detection for a batch with ONE CLASS LIST PER IMAGE, as one forward: images are HWC uint8 RGB arrays
    or paths, class_lists[i] the class names of image i (or a closed_set.ClassPrompt).  -> [(boxes xyxy [k, 4] in the
    pixels of the original image - normalised with normalized=True -, scores [k] descending, labels int64 [k] indexing
    class_lists[i])], k = min(num_select, num_queries * len(classes)): PostProcessCocoGrounding's result
    (GD/demo/test_ap_on_coco.py:66-137) with the image's own classes.  Stateless like predict."""
    images, class_lists = list(images), list(class_lists)
    if len(images) != len(class_lists):
        raise ValueError(f"{len(images)} images for {len(class_lists)} class lists: one class list per image")
    if not images:
        return []
    prompts = [_class_prompt(model, c) for c in class_lists]
    loaded = [_load_resized(model, im) for im in images]
    with _held_text(model):
        _set_prompts(model, prompts)
        maps = [p.positive_map for p in prompts]
        return model.predict_classes([r for r, _ in loaded], maps, num_select,
                                     None if normalized else [s for _, s in loaded])


def predict_classes(model, image, classes, num_select=300, normalized=False):
    """Closed-set detection of one image: which of `classes` is each box.  See predict_classes_batch."""
    return predict_classes_batch(model, [image], [classes], num_select, normalized)[0]


def predict_spans(model, image, caption, token_spans, box_threshold):
    """The given-phrase mode of the reference's demo (GD/demo/inference_on_a_image.py:117-142): token_spans is one list
    of (start, end) character spans per phrase, positions in the caption as predict preprocesses it (lower-cased,
    stripped, a trailing ".").  -> (boxes [n, 4] cxcywh normalised, scores [n], phrases [n]): for every phrase, in
    order, the queries whose phrase score exceeds box_threshold, each with the phrase's text.  Needs the vocabulary.
    Stateless like predict."""
    from inklayer_amd import closed_set
    prompt = closed_set.span_prompt(get_tokenizer(), caption, token_spans, model.cfg.max_text_len)
    resized, _ = _load_resized(model, image)
    with _held_text(model):
        _set_prompts(model, [prompt])
        boxes, scores, which = model.predict_spans([resized], prompt.positive_map, box_threshold)[0]
    return boxes, scores, [prompt.names[i] for i in which.tolist()]


def run_gdino_on_sketch_classes(sketch_path, nouns, score_threshold=0.2, num_select=300):
    """The reference's closed-set detector call (InkLayer/detector/gdino_mmdetection.py:25-98:
    run_ft_dino_inference_on_image(image_path, nouns, ...)) on this engine: {"bboxes": normalised xyxy lists, "labels":
    nouns[label] per box, "scores"}: the best num_select (query, class) pairs with a score >= score_threshold, best
    first."""
    boxes, scores, labels = predict_classes(get_model(), sketch_path, nouns, num_select, normalized=True)
    names = nouns.names if hasattr(nouns, "names") else list(nouns)
    keep = scores >= score_threshold
    return {"bboxes": boxes[keep].tolist(), "labels": [names[i] for i in labels[keep].tolist()],
            "scores": scores[keep].tolist()}


def run_gdino_on_sketches(paths, captions, box_threshold=0.2, text_threshold=0.0):
    """run_gdino_on_sketch for a batch of sketches, each with its own caption: a list of run_ft_dino_on_sketch-shaped
    dicts, in input order."""
    out = []
    for boxes, scores, phrases in predict_batch(get_model(), paths, captions, box_threshold, text_threshold):
        normalized = cxcywh_to_xyxy(boxes.tolist()).tolist()
        out.append({"bboxes": normalized, "scores": scores.tolist(), "labels": list(phrases)})
    return out


def run_gdino_on_sketch(sketch_path, caption, box_threshold=0.2, text_threshold=0.0):
    """run_ft_dino_on_sketch's dict for any caption: {"bboxes": normalised xyxy lists, "scores", "labels": the phrase of
    each box}."""
    boxes, scores, phrases = predict(get_model(), sketch_path, caption, box_threshold, text_threshold)
    normalized = cxcywh_to_xyxy(boxes.tolist()).tolist()
    return {"bboxes": normalized, "scores": scores.tolist(), "labels": list(phrases)}
