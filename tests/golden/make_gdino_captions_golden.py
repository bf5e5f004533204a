"""Generate tests/golden/gdino_captions_small.npz: the REFERENCE's Transformer on a batch of two images with two
captions of different length (build container only; a sibling of make_gdino_golden.py, whose stubs, imports and
weight recipe it re-uses by importing that module).  Nothing is written into /root/reference.

Batch: the image stored in gdino_small.npz and its horizontal flip (no new image is stored); captions of 23 ids and of
9 ids, the second padded with id 0 to 23 as the tokenizer's padding="longest" does (groundingdino.py:247-249).
text_token_mask, the self-attention masks and the position ids come from the reference's
generate_masks_with_special_tokens_and_transfer_map on the padded ids; the text features are seeded random [23, 256]
per image (the pad rows of image 1 hold random numbers too: nothing may depend on them).  The self-attention masks
reach the text enhancer expanded per head in batch-major order, and the modules run in float64 (results stored as
float32), see main() for both.  The forward is
GroundingDINO.forward (groundingdino.py:300-349) assembled from the reference's modules as in make_gdino_golden.py.
"""
import types
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

import make_gdino_golden as base          # installs the stubs and imports the reference's modules
from make_gdino_golden import (ContrastiveEmbed, MLP, NestedTensor, PositionEmbeddingSineHW, build_swin_transformer,
                               build_transformer, generate_masks_with_special_tokens_and_transfer_map, inverse_sigmoid,
                               load_prefixed)
from oracle import gdino_ref, sam_ref

IDS23 = [101, 2001, 2002, 2003, 2004, 2005, 2006, 1012, 3001, 3002, 3003, 3004, 3005, 3006, 3007, 3008, 1012,
         4001, 4002, 4003, 4004, 1012, 102]
IDS9 = [101, 2001, 2002, 1012, 3001, 1012, 4001, 1012, 102]


@torch.no_grad()
def main():
    cfg = base.SMALL
    sd = sam_ref.seeded_state_dict(gdino_ref.gdino_param_shapes(cfg), base.SEED)
    for k in sd:
        if k.endswith("gamma_v") or k.endswith("gamma_l"):
            sd[k] = 0.3 * torch.ones_like(sd[k]) + 0.05 * sd[k]
    args = types.SimpleNamespace(
        hidden_dim=cfg.hidden_dim, dropout=0.0, nheads=cfg.nheads, num_queries=cfg.num_queries,
        dim_feedforward=cfg.dim_feedforward, enc_layers=cfg.enc_layers, dec_layers=cfg.dec_layers,
        pre_norm=False, query_dim=4, transformer_activation="relu", num_patterns=0,
        num_feature_levels=4, enc_n_points=4, dec_n_points=4, two_stage_type="standard",
        embed_init_tgt=True, use_text_enhancer=True, use_fusion_layer=True, use_checkpoint=False,
        use_transformer_ckpt=False, use_text_cross_attention=True, text_dropout=0.0,
        fusion_dropout=0.0, fusion_droppath=0.1)
    swin = build_swin_transformer("swin_T_224_1k", 224, out_indices=(1, 2, 3), dilation=False, use_checkpoint=False)
    swin.eval()
    load_prefixed(swin, sd, "backbone.0.")
    posemb = PositionEmbeddingSineHW(128, temperatureH=20, temperatureW=20, normalize=True)
    tr = build_transformer(args)
    tr.eval()
    bbox = MLP(256, 256, 4, 3)
    load_prefixed(bbox, sd, "bbox_embed.0.")
    tr.enc_out_bbox_embed = MLP(256, 256, 4, 3)
    tr.enc_out_class_embed = ContrastiveEmbed()
    tr.decoder.bbox_embed = nn.ModuleList([bbox for _ in range(cfg.dec_layers)])
    tr.decoder.class_embed = nn.ModuleList([ContrastiveEmbed() for _ in range(cfg.dec_layers)])
    sub = {k[len("transformer."):]: v for k, v in sd.items() if k.startswith("transformer.")}
    for i in range(cfg.dec_layers):
        for j in range(3):
            for n in ("weight", "bias"):
                sub[f"decoder.bbox_embed.{i}.layers.{j}.{n}"] = sd[f"bbox_embed.0.layers.{j}.{n}"]
    tr.load_state_dict(sub, strict=True)
    inproj = nn.ModuleList([nn.Sequential(nn.Conv2d(c, 256, 1), nn.GroupNorm(32, 256)) for c in (192, 384, 768)]
                           + [nn.Sequential(nn.Conv2d(768, 256, 3, stride=2, padding=1), nn.GroupNorm(32, 256))])
    load_prefixed(inproj, sd, "input_proj.")
    # float64 throughout (the weights are the float32 numbers, widened).  In float32 this comparison has a floor of its
    # own: with these random weights a few queries are ill-conditioned, and torch's CPU kernels sum in another order at
    # B = 2 than at B = 1 - oracle/gdino_ref.py itself moves by 1.5e-4 of the logits' range (90th percentile) between the
    # two batch sizes, three times test_oracle_gdino's bound.  In float64 that movement is 1e-9 and the test that reads
    # this file (an image alone against its entry of this padded batch) holds the bound on the masks' arithmetic alone.
    for mod in (swin, tr, bbox, inproj):
        mod.double()

    img0 = torch.from_numpy(np.load(Path(__file__).with_name("gdino_small.npz"))["image"])      # [1, 3, 200, 264]
    img = torch.cat([img0, img0.flip(-1)]).contiguous().double()
    B, (h, w) = 2, img.shape[-2:]
    T = len(IDS23)
    ids = torch.tensor([IDS23, IDS9 + [0] * (T - len(IDS9))])
    t_len = [len(IDS23), len(IDS9)]
    token_mask = ids != 0                                       # attention_mask of the padded batch
    rs = np.random.RandomState(31)
    enc_text = torch.from_numpy((0.5 * rs.standard_normal((B, T, 256))).astype(np.float32))
    self_mask, pos_ids, _ = generate_masks_with_special_tokens_and_transfer_map(
        {"input_ids": ids}, [101, 102, 1012, 1029], None)
    # The text enhancer expands a [B, T, T] mask with src_mask.repeat(nhead, 1, 1) (transformer_vanilla.py:108-111): HEAD-
    # major rows, where nn.MultiheadAttention reads its [B * nhead, T, T] mask BATCH-major (row b * nhead + h).  With
    # B > 1 and masks that differ between the images, head h of image b would get the mask of image (b * nhead + h) % B
    # - an image's text would depend on its neighbours' captions (measured here: memory_text off by its own magnitude).
    # With equal masks, the only case the reference's callers exercise, both orders agree.  So the masks the
    # reference's generator made are handed over already expanded, batch-major, in the layout nn.MultiheadAttention
    # documents; the [B * nhead, T, T] shape passes the repeat untouched and every head of image b sees image b's mask.
    text_dict = {"encoded_text": enc_text.double(), "text_token_mask": token_mask, "position_ids": pos_ids,
                 "text_self_attention_masks": self_mask.repeat_interleave(tr.encoder.text_layers[0].nhead, 0)}

    mask = torch.zeros((B, h, w), dtype=torch.bool)
    feats = swin(NestedTensor(img, mask))
    features = [feats[i] for i in range(3)]
    poss = [posemb(f).to(f.tensors.dtype) for f in features]
    srcs, masks = [], []
    for l, f in enumerate(features):
        s, m = f.decompose()
        srcs.append(inproj[l](s))
        masks.append(m)
    s = inproj[3](features[-1].tensors)
    m = torch.nn.functional.interpolate(mask[None].float(), size=s.shape[-2:]).to(torch.bool)[0]
    poss.append(posemb(NestedTensor(s, m)).to(s.dtype))
    srcs.append(s)
    masks.append(m)
    hs, reference, _, _, _ = tr(srcs, masks, None, poss, None, None, text_dict)
    layer_hs, layer_ref = hs[-1], reference[:-1][-1]
    boxes = (bbox(layer_hs) + inverse_sigmoid(layer_ref)).sigmoid()
    logits = ContrastiveEmbed()(layer_hs, text_dict)            # [B, nq, 256], -inf at every masked column
    memory_text = text_dict["encoded_text"]                     # transformer.py:279 leaves the encoder's text here
    for b in range(B):
        assert torch.isfinite(logits[b, :, :t_len[b]]).all() and torch.isinf(logits[b, :, t_len[b]:]).all()
        assert torch.isfinite(memory_text[b, :t_len[b]]).all() and torch.isfinite(boxes[b]).all()

    out = dict(
        seed=np.int64(base.SEED), token_ids=ids.numpy().astype(np.int32), t_len=np.array(t_len, dtype=np.int32),
        text_token_mask=token_mask.numpy(), self_mask=self_mask.numpy(), position_ids=pos_ids.numpy().astype(np.int32),
        encoded_text=enc_text.numpy(), memory_text=memory_text.float().numpy(),
        pred_logits=logits[:, :, :T].float().numpy(), pred_boxes=boxes.float().numpy(),
        logits_past_longest_is_neginf=np.bool_(torch.isinf(logits[:, :, T:]).all().item()),
    )
    path = Path(__file__).with_name("gdino_captions_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, path.stat().st_size >> 10, "KiB")


if __name__ == "__main__":
    main()
