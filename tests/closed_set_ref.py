"""Plain restatements of the reference's closed-set post-processing, for the tests of inklayer_amd/closed_set.py,
ops.class_scores / ops.select_boxes and GDinoEngine.predict_classes / predict_spans.  Written from the reference's
lines, independent of the code under test (nothing of inklayer_amd is imported here):

  post_process          PostProcessCocoGrounding.forward, GD/demo/test_ap_on_coco.py:99-137, in float64
  class_scores_f32      its first three lines in float32 torch on the CPU - the reference's OWN arithmetic, whose distance
                        from float64 is the yardstick of the kernel's tolerance
  phrase_filter         the given-phrase mode, GD/demo/inference_on_a_image.py:124-142, in float64
  build_captions_and_token_span / create_positive_map_from_span     GD/util/vl_utils.py:49-87 and :8-46 in plain Python
                        (no random "/" alternative, no debug switch; char_to_token is a function argument)
"""
import torch


def class_scores_f64(logits, positive_map):
    """test_ap_on_coco.py:103-106: sigmoid(logits) @ positive_map.T; logits [..., nq, T], positive_map [C, T]."""
    return logits.double().sigmoid() @ positive_map.double().T


def class_scores_f32(logits, positive_map):
    return logits.float().sigmoid() @ positive_map.float().T


def box_cxcywh_to_xyxy(x):
    """GD/util/box_ops.py:10-13."""
    x_c, y_c, w, h = x.unbind(-1)
    return torch.stack([(x_c - 0.5 * w), (y_c - 0.5 * h), (x_c + 0.5 * w), (y_c + 0.5 * h)], dim=-1)


def post_process(logits, boxes, positive_map, target_sizes, num_select=300, dtype=torch.float64):
    """PostProcessCocoGrounding.forward for logits [B, nq, T], boxes [B, nq, 4] cxcywh, positive_map [C, T],
    target_sizes [B, 2] = (h, w) -> per image dict(scores, labels, boxes, query), best first; ties to the lower flat
    (query, class) index (a stable sort: torch.topk leaves the order of ties open)."""
    prob = logits.to(dtype).sigmoid() @ positive_map.to(dtype).T
    B, nq, C = prob.shape
    k = min(num_select, nq * C)
    order = torch.sort(prob.view(B, -1), dim=1, descending=True, stable=True)[1][:, :k]
    scores = torch.gather(prob.view(B, -1), 1, order)
    topk_boxes, labels = order // C, order % C
    xyxy = box_cxcywh_to_xyxy(boxes.to(dtype))
    xyxy = torch.gather(xyxy, 1, topk_boxes.unsqueeze(-1).repeat(1, 1, 4))
    img_h, img_w = target_sizes.to(dtype).unbind(1)
    xyxy = xyxy * torch.stack([img_w, img_h, img_w, img_h], dim=1)[:, None, :]
    return [dict(scores=s, labels=l, boxes=b, query=q) for s, l, b, q in zip(scores, labels, xyxy, topk_boxes)]


def phrase_filter(logits, boxes, positive_map, box_threshold):
    """inference_on_a_image.py:124-142 for ONE image: logits [nq, T], boxes [nq, 4], positive_map [P, T] ->
    (boxes [n, 4], scores [n], phrase index [n]): phrase by phrase, the queries above the threshold in query order."""
    per_phrase = positive_map.double() @ logits.double().sigmoid().T           # [P, nq]
    all_boxes, all_scores, which = [], [], []
    for p, row in enumerate(per_phrase):
        keep = row > box_threshold
        all_boxes.append(boxes[keep])
        all_scores.append(row[keep])
        which.append(torch.full((int(keep.sum()),), p, dtype=torch.int64))
    return torch.cat(all_boxes), torch.cat(all_scores), torch.cat(which)


def build_captions_and_token_span(cat_list, force_lowercase=True):
    """vl_utils.py:49-87 -> (caption, [spans of each class, in order])."""
    captions, spans = "", []
    for catname in cat_list:
        class_name = catname.lower() if force_lowercase else catname
        tokens_positive_i = []
        for subname in [i.strip() for i in class_name.strip().split(" ")]:
            if len(subname) == 0:
                continue
            if len(captions) > 0:
                captions = captions + " "
            start = len(captions)
            tokens_positive_i.append([start, start + len(subname)])
            captions = captions + subname
        if len(tokens_positive_i) > 0:
            captions = captions + " ."
        spans.append(tokens_positive_i)
    return captions, spans


def create_positive_map_from_span(char_to_token, token_span, max_text_len=256):
    """vl_utils.py:8-46; char_to_token(i) -> token index or None."""
    positive_map = torch.zeros((len(token_span), max_text_len), dtype=torch.float)
    for j, tok_list in enumerate(token_span):
        for (beg, end) in tok_list:
            beg_pos = char_to_token(beg)
            end_pos = char_to_token(end - 1)
            if beg_pos is None:
                beg_pos = char_to_token(beg + 1)
                if beg_pos is None:
                    beg_pos = char_to_token(beg + 2)
            if end_pos is None:
                end_pos = char_to_token(end - 2)
                if end_pos is None:
                    end_pos = char_to_token(end - 3)
            if beg_pos is None or end_pos is None:
                continue
            positive_map[j, beg_pos: end_pos + 1].fill_(1)
    return positive_map / (positive_map.sum(-1)[:, None] + 1e-6)
