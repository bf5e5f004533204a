"""GroundingDINO's text branch on the GPU: feat_map(BERT(captions)) for a batch of captions in ONE pass.

The host fold (inklayer_amd/text_branch.py) encodes one caption at a time in f32 torch on the CPU; it stays the path of
the load-time constant "object." and of engines without a GPU.  With one caption per image (GDinoEngine.set_captions)
the text features are on the hot path, and this module runs the same forward - BertModelWarper.forward,
GD/.../bertwarper.py:31-166: HF BertModel with the sub-sentence block mask and per-phrase position ids, then
groundingdino.py:277-279's feat_map - on the library's kernels for all captions at once, packed row after row:

    embeddings   ops.text_embed_ln              word + position + type rows, LayerNorm        (csrc/text_bert.hip)
    per layer    ops.gemm                       fused query | key | value projection, f32 out
                 ops.attn_text_f32              12 heads x 64 on f32 rows, block mask          (csrc/text_bert.hip)
                 ops.gemm                       attention.output.dense
                 ops.layernorm_rows (add)       attention.output.LayerNorm(. + x) -> split operand + f32 copy
                 ops.gemm (gelu)                intermediate.dense
                 ops.add_split_f16              its operand form
                 ops.gemm                       output.dense
                 ops.layernorm_rows (add)       output.LayerNorm(. + x) -> split operand + f32 copy
    feat_map     ops.gemm (row_map)             [R, 768] -> [.., 256], optionally scattered into padded rows

Every product runs on split-f16 operands (~2^-21 relative, against the reference's fp32), 8 launches
per layer and 2 around them; there is no host synchronisation inside a pass (the ids, position ids, masks and row
tables of a call are built on the host and uploaded before its first launch).

The residual of the two output projections is added by the LayerNorm that follows (its `add` row), not by the GEMM's
residual epilogue: that epilogue preloads the residual into the accumulators, so each of the 72 to 288 MFMA steps of a
split-f16 product then rounds at the residual's magnitude (up to 4) instead of the partial sum's.  Measured on an
MI355X against float64, 2-layer model: 1.06e-5 with the epilogue against 2.4e-6 with the LayerNorm's addend, the host
f32 fold at 1.1e-6 ("Caption encoder")."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch

from . import ops
from .gdino import clean_state_dict, text_masks_and_position_ids

F32, I32 = torch.float32, torch.int32
HIDDEN, HEADS = 768, 12


def bert_hidden_size(sd: Dict[str, torch.Tensor]) -> int:
    """Hidden size of the `bert.*` tensors in sd (0: there is no BERT in it)."""
    w = sd.get("bert.embeddings.word_embeddings.weight")
    return int(w.shape[1]) if w is not None and w.dim() == 2 else 0


class BertTextEncoder:
    """feat_map(BERT(.)) of the checkpoint's `bert.*` / `feat_map.*` tensors on device `dev`, see the module text."""

    def __init__(self, sd: Dict[str, torch.Tensor], dev):
        sd, self.dev = clean_state_dict(sd), torch.device(dev)
        if self.dev.type != "cuda":
            raise ValueError("BertTextEncoder runs on a GPU (the host fold is inklayer_amd.text_branch)")
        if bert_hidden_size(sd) != HIDDEN:
            raise ValueError(f"BertTextEncoder serves BERT-base's {HIDDEN} hidden units ({HEADS} heads x 64), "
                             f"not {bert_hidden_size(sd)}")
        f = lambda k: ops.own_f32(sd[k], self.dev)
        sw = lambda w: ops.split_weight(w.detach().to(self.dev, F32))       # the load-time re-layout, done on the device
        e = "bert.embeddings."
        self.word, self.pos = f(e + "word_embeddings.weight"), f(e + "position_embeddings.weight")
        self.type_row = f(e + "token_type_embeddings.weight")[0].clone()
        self.emb_g, self.emb_b = f(e + "LayerNorm.weight"), f(e + "LayerNorm.bias")
        self.vocab_size, self.max_positions = self.word.shape[0], self.pos.shape[0]
        self.n_layers = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith("bert.encoder.layer."))
        self.layers: List[Dict[str, torch.Tensor]] = []
        for i in range(self.n_layers):
            p = f"bert.encoder.layer.{i}."
            qkv = [p + "attention.self." + n for n in ("query", "key", "value")]
            self.layers.append({
                "qkv_w": sw(torch.cat([sd[n + ".weight"].detach().to(F32) for n in qkv], 0)),
                "qkv_b": ops.own_f32(torch.cat([sd[n + ".bias"].detach().to(F32) for n in qkv], 0), self.dev),
                "ao_w": sw(sd[p + "attention.output.dense.weight"]), "ao_b": f(p + "attention.output.dense.bias"),
                "ln1_g": f(p + "attention.output.LayerNorm.weight"), "ln1_b": f(p + "attention.output.LayerNorm.bias"),
                "in_w": sw(sd[p + "intermediate.dense.weight"]), "in_b": f(p + "intermediate.dense.bias"),
                "out_w": sw(sd[p + "output.dense.weight"]), "out_b": f(p + "output.dense.bias"),
                "ln2_g": f(p + "output.LayerNorm.weight"), "ln2_b": f(p + "output.LayerNorm.bias"),
            })
        self.intermediate_size = self.layers[0]["in_b"].numel()
        self.fm_w, self.fm_b = sw(sd["feat_map.weight"]), f("feat_map.bias")
        self.out_dim = self.fm_b.numel()

    @property
    def nbytes(self) -> int:
        ts = [self.word, self.pos, self.type_row, self.emb_g, self.emb_b, self.fm_w, self.fm_b]
        ts += [t for l in self.layers for t in l.values()]
        return sum(t.numel() * t.element_size() for t in ts)

    launches_per_pass = property(lambda self: 2 + 8 * self.n_layers)

    def _tables(self, id_lists: Sequence[Sequence[int]]):
        """Host side of a pass: packed ids and position ids, the row table and the masks, checked, then uploaded."""
        caps = [[int(t) for t in ids] for ids in id_lists]
        if not caps or any(len(c) < 1 for c in caps):
            raise ValueError("at least one caption, each of at least one token id")
        Tmax = max(len(c) for c in caps)
        if Tmax > 256:
            raise ValueError(f"a caption of {Tmax} tokens: the text attention takes at most 256")
        if any(t < 0 or t >= self.vocab_size for c in caps for t in c):
            raise ValueError(f"token id outside 0..{self.vocab_size - 1}")
        B = len(caps)
        blocked = torch.ones(B, Tmax, Tmax, dtype=torch.bool)
        pos, starts = [], [0]
        for b, c in enumerate(caps):
            sm, p = text_masks_and_position_ids(c)
            blocked[b, :len(c), :len(c)] = ~sm
            pos.append(p)
            starts.append(starts[-1] + len(c))
        pos = torch.cat(pos)
        if int(pos.max()) >= self.max_positions:
            raise ValueError(f"position id outside 0..{self.max_positions - 1}")
        up = lambda t, dt: t.to(dt).to(self.dev)
        ids = torch.tensor([t for c in caps for t in c], dtype=torch.int64)
        return (caps, Tmax, up(ids, I32), up(pos, I32), up(torch.tensor(starts), I32), up(blocked, torch.uint8).contiguous())

    def _layers(self, id_lists) -> Tuple[List[List[int]], torch.Tensor, torch.Tensor]:
        caps, Tmax, ids, pos, row_start, blocked = self._tables(id_lists)
        x, xs = ops.text_embed_ln(ids, pos, self.word, self.pos, self.type_row, self.emb_g, self.emb_b, 1e-12)
        R = x.shape[0]
        y = torch.empty_like(x)
        for l in self.layers:
            qkv = ops.gemm(xs, l["qkv_w"], l["qkv_b"])                                    # [R, 2304] f32
            ctx, _ = ops.attn_text_f32(qkv[:, :HIDDEN], qkv[:, HIDDEN:2 * HIDDEN], qkv[:, 2 * HIDDEN:], row_start,
                                       Tmax=Tmax, n_heads=HEADS, scale=0.125, blocked=blocked)
            a = ops.gemm(ctx, l["ao_w"], l["ao_b"])
            xs = ops.layernorm_rows(a, l["ln1_g"], l["ln1_b"], 1e-12, split=True, split_f32=y, add=x)
            mid = ops.gemm(xs, l["in_w"], l["in_b"], act="gelu")                          # [R, 3072] f32
            o = ops.gemm(ops.add_split_f16(mid), l["out_w"], l["out_b"])
            xs = ops.layernorm_rows(o, l["ln2_g"], l["ln2_b"], 1e-12, split=True, split_f32=x, add=y)
        assert x.shape[0] == R
        return caps, x, xs

    @torch.no_grad()
    def hidden(self, id_lists: Sequence[Sequence[int]]) -> torch.Tensor:
        """BERT's last_hidden_state of every caption, packed: f32 [sum T_b, 768] on the device."""
        return self._layers(id_lists)[1]

    @torch.no_grad()
    def encode(self, id_lists: Sequence[Sequence[int]]) -> List[torch.Tensor]:
        """feat_map(BERT(ids)) per caption: a list of f32 [T_b, 256] device tensors (views of one packed result)."""
        caps, _, xs = self._layers(id_lists)
        out = ops.gemm(xs, self.fm_w, self.fm_b)
        return list(out.split([len(c) for c in caps], 0))

    @torch.no_grad()
    def encode_into(self, id_lists: Sequence[Sequence[int]], out: torch.Tensor, Tmax: int) -> torch.Tensor:
        """The same rows written straight into `out`, a ZEROED f32 [B * Tmax, 256] buffer: caption b's token t lands
        in row b * Tmax + t through the feat_map GEMM's row_map; the pad rows are not touched."""
        lens = [len(c) for c in id_lists]
        assert out.dtype == F32 and out.is_contiguous() and tuple(out.shape) == (len(lens) * Tmax, self.out_dim)
        assert out.device == self.dev and 1 <= min(lens) and max(lens) <= Tmax
        rows = torch.cat([b * Tmax + torch.arange(n) for b, n in enumerate(lens)]).to(I32).to(self.dev)
        xs = self._layers(id_lists)[2]
        ops.gemm(xs, self.fm_w, self.fm_b, row_map=rows, out=out)
        return out
