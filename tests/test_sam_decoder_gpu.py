"""float64 parity of the SAM prompt encoder + mask decoder as SamEngine.decode_prompts / _decode_tokens_split compose
them, seam by seam, on depth-0 engines with dec_depth = 2 and dec_depth = 1 (layer 0's shared keys followed directly by the
final attention).  The seams are captured without touching sam.py: inklayer_amd.ops' sam_prompt_tokens, add_f32 /
sam_mask_embed, layernorm_rows (call order: norm1 / norm2 / norm3 per layer, then norm_final_attn), proj256_ln and
sam_upscale_tail (its hyper argument) are wrapped to record clones and pass through; the call counts are asserted, so a
reordered engine fails loudly and no seam is mislabelled.  The last layer's keys exist only as the split operand
[hi | lo * 64 | hi / 64]: hi + lo / 64 is rebuilt in float64 and the third segment must be f16(hi / 64) bitwise.

Cases, references, the yardstick and the named mistakes are in tests/sam_decoder_ref.py: at every seam, per prompt and
over the whole tensor, at every quantile including the maximum, HIP error against float64 <= 8 x the error of the same
restatement in float32; nothing is exempt.  tests/test_sam_decoder_ref_cpu.py shows on the CPU that this bound tells every
named mistake apart (>= 10x) and stays 16x below f16-operand grade.  GPU box only.

The iou seam ([n, M], M <= 4) has too few numbers per group for quantiles of their own; such groups are held element by
element to the pooled bound of sam_decoder_ref.MIN_POP (reasoning there).

Measured on an MI355X at 49e00b4 + this change; worst HIP error / bound over all cases, prompts and quantiles, per seam:
  dec_depth 2: tokens 0.261 (C1)  keys0 0.324 (E, the mask embedding; 0.125 without a mask)  q_norm1.0 0.313 (B)
               q_norm2.0 0.317 (G5)  q_norm3.0 0.416 (B)  keys_norm4.0 0.275 (B)  q_norm1.1 0.437 (B)  q_norm2.1 0.347 (B)
               q_norm3.1 0.509 (B)  keys_norm4.1 0.257 (GA)  q_final 0.483 (C10)  hyper 0.384 (F0)  iou 0.268 (B)
               low 0.276 (C1)
  dec_depth 1: tokens 0.251  keys0 0.125  q_norm1.0 0.313  q_norm2.0 0.317  q_norm3.0 0.416  keys_norm4.0 0.294 (from the
               split operand)  q_final 0.407  hyper 0.360  iou 0.212  low 0.245
The medians sit at 0.13 - 0.21 of the bound (HIP median error 2e-7 .. 4e-7: 1 - 1.7 x the float32 evaluation's).  The
permuted call and every prompt alone are bit-equal to the batch at all 14 seams; so is a call after calls of other shapes.

What these tests found, and what was changed for it.  With lin2 of the token MLP taking its residual in the GEMM (as the
engine did before), q_norm3 sat at 0.79 - 0.90 of the bound in four cases and case C10 left it: q_final of prompt 1 at the
maximum, HIP 9.90e-6 against 9.63e-6 (1.028; q0.999 at 0.42).  The element left the crowd at q_norm3.1 (largest error
3.4e-6 at q_norm2.1, 9.5e-6 at q_norm3.1) and rode the residual into q_final.  At op level, on the recorded operands of
that call: lin2 - the split GEMM at K = 2048, K' = 6144 f16 products in one MFMA accumulation chain of 192 steps - was up to
1.10e-5 (sigma 9.1e-7) off the exact product OF ITS OWN f16 OPERANDS, layer 0's 6.0e-6; the K = 256 GEMMs sigma 1.6e-7, the
LayerNorms 5e-7 at most.  An IEEE float32 chain over the same 32-wide steps is 2.1e-6 (sigma 2.7e-7) off when it starts
from zero and 3.1e-6 (sigma 4.4e-7) when it starts from the residual, as the kernel's did: the GEMM preloads the residual
into the accumulator, its worst elements were those with |residual| of 4 - 5, where every one of the 192 steps rounds at
that ulp (peak |accumulator| 4 - 5 against 1 - 3 from zero).  The split operands are not the cause: emulated inside the
float64 restatement (sam_decoder_ref.split_operands) they give 5.6e-7 at most at q_final, so the bound stayed at 8 x.
The composition was changed instead: lin2 runs without a residual and norm3 adds it (layernorm_rows(add=)), the same
number of launches.  q_norm3 is now at 0.42 / 0.51, q_final at 0.48, and every later seam moved down with them."""
import numpy as np
import pytest
import torch

import encoder_ends_ref as Y
import sam_decoder_ref as R

pytestmark = pytest.mark.gpu

T, E = R.T, R.E
_ENGINES = {}
WRAPPED = ("sam_prompt_tokens", "add_f32", "sam_mask_embed", "layernorm_rows", "proj256_ln", "sam_upscale_tail")


def _engine(dev, depth, small=False):
    """Depth-0 encoder, seeded decoder weights (seed 11; small: case G's state dict), bias_correction off."""
    from inklayer_amd import sam
    if (depth, small) not in _ENGINES:
        cfg = sam.SamConfig(depth=0, global_attn_indexes=(), dec_depth=depth)
        _ENGINES[depth, small] = sam.SamEngine(R.state_dict(R.F32, small), cfg, dev, max_batch=1, bias_correction=False)
    return _ENGINES[depth, small]


def _split_to_f64(osp):
    """[R, 3E] split operand -> float64 hi + lo / 64; the third segment is f16(hi / 64) bitwise."""
    hi, lo, h64 = osp[:, :E], osp[:, E:2 * E], osp[:, 2 * E:]
    assert torch.equal(h64, (hi.float() / 64).half()), "third segment of the split operand is not f16(hi / 64)"
    return hi.double() + lo.double() / 64


def _decode(dev, monkeypatch, depth, c, rows=None):
    """eng.decode_prompts on case dict c (rows: a selection / permutation of its prompts) with the taps on -> {seam: f64
    or f32 CPU tensor}, shaped as sam_decoder_ref.decoder's."""
    from inklayer_amd import ops
    eng = _engine(dev, depth, c["small"])
    rec = {k: [] for k in WRAPPED}

    def keep(x):
        return None if x is None else tuple(keep(y) for y in x) if isinstance(x, tuple) else x.detach().clone()

    def wrap(name):
        real = getattr(ops, name)

        def f(*a, **kw):
            out = real(*a, **kw)
            rec[name].append((keep(out), keep(kw.get("hyper", a[8])) if name == "sam_upscale_tail" else None))
            return out
        return f

    sel = list(range(len(c["img"]))) if rows is None else list(rows)
    pick = lambda t: None if t is None else t[sel].contiguous()
    img = [c["img"][p] for p in sel]
    with monkeypatch.context() as mp:
        for name in WRAPPED:
            mp.setattr(ops, name, wrap(name))
        low, iou = eng.decode_prompts(c["emb"].to(dev), img, pick(c["points"]), pick(c["labels"]), pick(c["boxes"]),
                                      pick(c["mask_input"]), masks=c["masks"])
        torch.cuda.synchronize()
    n, has_mask = len(sel), c["mask_input"] is not None
    counts = {k: len(v) for k, v in rec.items()}
    assert counts == {"sam_prompt_tokens": 1, "add_f32": 0 if has_mask else 1, "sam_mask_embed": 1 if has_mask else 0,
                      "layernorm_rows": 3 * depth + 1, "proj256_ln": depth, "sam_upscale_tail": 1}, counts
    got = {"tokens": rec["sam_prompt_tokens"][0][0]}
    NT = got["tokens"].shape[1]
    if has_mask:
        keys, ks = rec["sam_mask_embed"][0][0]
        got["keys0"] = keys.view(n, T, E)
        assert torch.equal(ks[:, :E], keys.half())
    else:
        shared = rec["add_f32"][0][0]
        assert tuple(shared.shape) == (c["emb"].shape[0] * T, E)      # one copy per image; the engine gathers per box
        got["keys0"] = shared.view(-1, T, E)[img]
    for i in range(depth):
        for j, s in enumerate(("q_norm1", "q_norm2", "q_norm3")):
            x = rec["layernorm_rows"][3 * i + j][0]
            assert x.dtype == torch.float32 and tuple(x.shape) == (n * NT, E), (s, i, x.shape)
            got[f"{s}.{i}"] = x.view(n, NT, E)
        of, osp = rec["proj256_ln"][i][0]
        last = i + 1 == depth
        assert (of is None) == last and osp is not None and tuple(osp.shape) == (n * T, 3 * E)
        got[f"keys_norm4.{i}"] = (_split_to_f64(osp) if last else of).view(n, T, E)
        if not last:          # the operand the next layer's projections read is the f32 keys, split
            assert torch.equal(osp[:, :E], of.half())
            assert (_split_to_f64(osp) - of.double()).abs().max().item() <= 2.0 ** -21 * of.abs().max().item()
    x = rec["layernorm_rows"][3 * depth][0]
    assert tuple(x.shape) == (n * NT, E)
    got["q_final"] = x.view(n, NT, E)
    got["hyper"] = rec["sam_upscale_tail"][0][1]
    M = c["masks"][1]
    assert tuple(got["hyper"].shape) == (n, M, 32) and tuple(low.shape) == (n, M, 256, 256) and tuple(iou.shape) == (n, M)
    got["iou"], got["low"] = iou, low
    return {k: v.cpu() for k, v in got.items()}


def _hold(got, cid, depth, rows=None, what="", overall=True):
    """Every seam of `got` (its prompt k is prompt rows[k] of the case) against the case's references: over the whole
    tensor (if overall) and per prompt.  Every figure is printed before anything is asserted.  -> {seam: worst ratio}."""
    ref, _ = R.refs(cid, depth)
    n = got["tokens"].shape[0]
    rows = list(range(n)) if rows is None else list(rows)
    worst, failures = {}, []
    for s in R.seam_names(depth):
        assert got[s].shape[1:] == ref[s].shape[1:], (s, got[s].shape, ref[s].shape)
        checks = [(f"{what}{cid} depth {depth} {s} prompt {p}", got[s][k], ref[s][p], R.bound(cid, depth, s, p))
                  for k, p in enumerate(rows)]
        if overall:
            assert rows == list(range(ref[s].shape[0]))
            checks.insert(0, (f"{what}{cid} depth {depth} {s} all", got[s], ref[s], R.bound(cid, depth, s)))
        w = 0.0
        for name, g, r, b in checks:
            if r.numel() < R.MIN_POP:          # too few numbers for quantiles of their own (sam_decoder_ref.MIN_POP)
                assert s == "iou", (s, r.shape)
                b = np.full(len(Y.QUANTILES), R.pooled_iou_bound(depth, R.CASES if depth == 2 else R.DEPTH1_CASES))
                name += " (pooled bound)"
            try:
                ratio = Y.assert_within(g, r, b, name)
            except AssertionError as e:
                failures.append(str(e)[:300])
                ratio = Y.quantiles((g.double() - r).abs()) / b
            with np.errstate(all="ignore"):
                ratio = np.where(np.isnan(ratio), 0.0, ratio)          # 0 / 0: both exact (the copied output tokens)
            w = max(w, float(ratio.max()))
        worst[s] = w
    print(f"WORST {what}{cid} depth {depth}: " + "  ".join(f"{s} {w:.3f}" for s, w in worst.items()))
    assert not failures, f"{len(failures)} seam checks outside the bound, first: {failures[:3]}"
    return worst


CASE_PARAMS = [(c, 2) for c in R.CASES] + [(c, 1) for c in R.DEPTH1_CASES]


@torch.no_grad()
@pytest.mark.parametrize("cid,depth", CASE_PARAMS, ids=[f"{c}-depth{d}" for c, d in CASE_PARAMS])
def test_seams_match_float64(dev, monkeypatch, cid, depth):
    """Every seam of every case, per prompt and overall, within 8 x the float32 restatement's own error."""
    _hold(_decode(dev, monkeypatch, depth, R.case(cid)), cid, depth)


@torch.no_grad()
def test_wrong_gathers_show_on_all_of_case_b():
    """The mistakes the CPU test ran on B's 3-prompt cut, on all 17 prompts and 4 images: keys or norm4 residual gathered
    from image (i + 1) % B, residual from box p - 1.  Per prompt and overall, >= 10x outside the bound of their first
    seam; the three prompts whose predecessor sits on the same image are untouched by 'box p-1' at that seam."""
    ref, _ = R.refs("B", 2)
    img = R.case("B")["img"]
    n = len(img)
    for m in ("t2i keys from image (i+1) % B", "norm4 residual from image (i+1) % B", "norm4 residual from box p-1"):
        first = R.MISTAKES[m]
        wrong = R.run("B", R.F64, 2, m, upto=first)[first]
        Y.assert_discriminates(wrong, ref[first], R.bound("B", 2, first), f"B {first}: {m}", R.reach("B", m))
        for p in range(n):
            if m.endswith("box p-1") and img[p] == img[p - 1]:
                assert torch.equal(wrong[p], ref[first][p])
                continue
            Y.assert_discriminates(wrong[p], ref[first][p], R.bound("B", 2, first, p), f"B {first} prompt {p}: {m}")
    assert R.reach("B", "norm4 residual from box p-1") == 14 / 17


def _bitwise(a, b, rows=None):
    same = [s for s in a if torch.equal(a[s], b[s] if rows is None else b[s][rows])]
    return f"bitwise equal at {len(same)} of {len(a)} seams" + ("" if len(same) == len(a) else
                                                                 f" (not at {[s for s in a if s not in same]})")


@torch.no_grad()
def test_permuting_prompts_permutes_every_seam(dev, monkeypatch):
    """Case B with its prompts permuted: prompt k of the permuted call is held to the reference of the prompt it is."""
    c = R.case("B")
    perm = np.random.RandomState(3).permutation(len(c["img"])).tolist()
    assert perm != sorted(perm)
    got = _decode(dev, monkeypatch, 2, c, rows=perm)
    _hold(got, "B", 2, rows=perm, what="permuted ", overall=False)
    print("permuted against the plain call: " + _bitwise(got, _decode(dev, monkeypatch, 2, c), perm))


@torch.no_grad()
def test_each_prompt_alone_matches_its_row(dev, monkeypatch):
    """Prompt p of case B alone (n = 1, B = 1, its own image) is held to the reference of its row in the batch."""
    c = R.case("B")
    batch = _decode(dev, monkeypatch, 2, c)
    for p, i in enumerate(c["img"]):
        one = dict(c, emb=c["emb"][i:i + 1], img=(0,) * len(c["img"]))
        got = _decode(dev, monkeypatch, 2, one, rows=[p])
        _hold(got, "B", 2, rows=[p], what="alone ", overall=False)
        print(f"prompt {p} alone against its row of the batch: " + _bitwise(got, batch, [p]))


@torch.no_grad()
def test_call_after_another_shape_gives_the_same_bits(dev, monkeypatch):
    """No workspace or cached row table of a call with another n / NT / B leaks into the next: B, then C10 (n = 2, NT = 16,
    B = 2) and E (mask input), then B again; A likewise around D11."""
    for cid, others in (("B", ("C10", "E")), ("A", ("D11", "B"))):
        first = _decode(dev, monkeypatch, 2, R.case(cid))
        for o in others:
            _decode(dev, monkeypatch, 2, R.case(o))
        again = _decode(dev, monkeypatch, 2, R.case(cid))
        for s in first:
            assert torch.equal(first[s], again[s]), (cid, s)


@torch.no_grad()
def test_mask_m_of_a_four_mask_call_is_the_one_mask_call(dev, monkeypatch):
    """Case F: masks = (m, 1) for m = 0 .. 3 and (1, 3) give the bits of the matching masks of (0, 4), at low, iou and
    hyper; every seam before the mask-token selection has the same bits in all six calls."""
    four = _decode(dev, monkeypatch, 2, R.case("F04"))
    for cid, lo, M in (("F0", 0, 1), ("F1", 1, 1), ("F2", 2, 1), ("F3", 3, 1), ("F13", 1, 3)):
        got = _decode(dev, monkeypatch, 2, R.case(cid))
        for s in got:
            want = four[s][:, lo:lo + M] if s in ("hyper", "iou", "low") else four[s]
            assert torch.equal(got[s], want), (cid, s)
