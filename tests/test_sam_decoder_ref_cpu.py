"""CPU side of tests/test_sam_decoder_gpu.py: the seam-by-seam restatement of tests/sam_decoder_ref.py is pinned to
tests/sam_prompt_ref.py (float64) and to oracle/sam_ref.py (float32, boxes), and every condition the GPU test only assumes
is asserted here on its own fixtures, on the cases A, C (N = 3), D (NT = 8), E, G and a 3-box / 2-image cut of B:
  * each named mistake, evaluated in float64, leaves every seam before its own untouched and lands >= 10x outside the
    bound of the seam it first reaches, at every quantile where it should show, in each case its geometry reaches; where
    the geometry does not reach, the mistake is a no-op (every seam bit-equal), so that the table itself is checked;
  * case G's variance condition;
  * the bound at `low` (8 x the float32 evaluation) stays <= 1/16 of the error of f16-rounded linear operands.

Reach of the mistakes (sam_decoder_ref.reach; share of the first seam's elements):
  +0.5 dropped                       tokens     the sparse tokens that carry a positional encoding (not label -1, not the pad)
  label -1 given the pe              tokens     label -1 points and the pad point: cases with points (C; D8 has none)
  box corners swapped                tokens     2 of NT tokens: cases with a box
  no_mask_embed dropped              keys0      all, without a mask input (not E)
  first conv taps transposed         keys0      E's prompt (a) alone: a constant map and 2x2 blocks are blind to it
  layer 0 self-attn + residual / pe  q_norm1.0  all
  k_pe dropped, pe added to v, scale q_norm2.0  all
  t2i keys from image (i+1) % B      q_norm2.0  shared keys and B > 1 (not A, GA, E)
  ReLU<->GELU                        q_norm3.0  all
  q_pe dropped                       keys_norm4.0  all
  norm4 residual from image (i+1)%B  keys_norm4.0  shared keys and B > 1 (not A, GA, E)
  norm4 residual from box p-1        keys_norm4.0  prompts whose predecessor has other keys (n > 1)
  layer 1 self-attn without pe       q_norm1.1  all at dec_depth 2, none at dec_depth 1
  hyper-network of token m+1         hyper      all
  IoU columns not shifted            iou        mask_lo > 0 (C, E)
  tanh-GELU in the upscaler          low        all
  (dy, dx) swapped, either ConvT     low        half: the sub-pixels with dy == dx of that convolution stay
  norm4 eps 1e-6, LN2d eps 1e-5      keys_norm4.0 / low   reach everything, decisive where the variance is near eps: G"""
import pytest
import torch

import encoder_ends_ref as Y
import sam_decoder_ref as R
import sam_prompt_ref as PR
from oracle import sam_ref as S

F32, F64 = R.F32, R.F64
EPS_MISTAKES = ("norm4 eps 1e-6", "LayerNorm2d eps 1e-5 in the upscaler")


@torch.no_grad()
@pytest.mark.parametrize("cid", R.CPU_CASES)
def test_restatement_matches_sam_prompt_ref(cid):
    """low and iou of every CPU case equal sam_prompt_ref.decode_all (all four mask tokens, then the selection) in
    float64 to 1e-12 relative, and the sparse tokens its embed_sparse."""
    c, cfg = R.case(cid), R.config()
    sd = R.state_dict(F64, c["small"])
    ref = R.refs(cid)[0]
    sparse = PR.embed_sparse(sd, cfg, c["points"], c["labels"], c["boxes"])
    assert (ref["tokens"][:, 5:] - sparse).abs().max().item() <= 1e-12
    emb = torch.stack([c["emb"][i].t().reshape(R.E, R.G, R.G) for i in c["img"]]).double()
    low, iou = PR.decode_all(sd, cfg, emb, sparse, c["mask_input"])
    lo, M = c["masks"]
    for got, want in ((ref["low"], low[:, lo:lo + M]), (ref["iou"], iou[:, lo:lo + M])):
        assert got.shape == want.shape
        assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


@torch.no_grad()
@pytest.mark.parametrize("cid", ["A", "Bcut", "G5"])
def test_restatement_matches_oracle_in_float32(cid):
    """The box cases against oracle.sam_ref.mask_decoder in float32, one prompt on its own image at a time as the oracle
    decodes.  Two float32 evaluations of one function differ by their rounding, which the decoder's depth amplifies (a few
    ulp of the largest logit), so "equal to float32 rounding" is held as: at every quantile the oracle's distance from the
    float64 restatement is <= 2 x the float32 restatement's own, and the two float32 results differ by no more than the
    sum of both maxima.  Any named mistake is >= 80x the float32 restatement's error."""
    c, cfg = R.case(cid), R.config()
    sd, sd64 = R.state_dict(F32, c["small"]), R.state_dict(F64, c["small"])
    pe = S.dense_pe(sd, cfg)
    for p, i in enumerate(c["img"]):
        box = c["boxes"][p:p + 1]
        got, ref = (R.decoder(w, cfg, c["emb"][i:i + 1], [0], boxes=box) for w in (sd, sd64))
        low, iou = S.mask_decoder(sd, cfg, c["emb"][i].t().reshape(1, R.E, R.G, R.G), pe, S.embed_boxes(sd, cfg, box))
        for name, want in (("low", low), ("iou", iou)):
            assert got[name].dtype == F32 and want.dtype == F32 and got[name].shape == want.shape
            mine, theirs = Y.quantiles((got[name].double() - ref[name]).abs()), Y.quantiles((want.double() - ref[name]).abs())
            diff = (got[name] - want).abs().max().item()
            print(f"  {cid} prompt {p} {name}: oracle / restatement float32 error " + " ".join(f"{x:.2f}" for x in theirs / mine)
                  + f", |restatement - oracle| max {diff:.2e}")
            assert diff <= mine[-1] + theirs[-1]
            if name == "low":                        # iou is a single number: its float32 error can be anything down to 0
                assert (theirs <= 2 * mine).all()


@torch.no_grad()
@pytest.mark.parametrize("cid", ["GA", "G5"])
def test_case_g_variance_condition(cid):
    """The median row variance entering layer 0's norm4 in float64 lies in [1e-5, 1e-3] (eps is 1e-5), and so does the
    variance the upscaler's LayerNorm2d (eps 1e-6) sees; in case A both are O(1), which is why G exists."""
    ref = R.refs(cid)[0]
    v4, vu = ref["_var4.0"].median().item(), ref["_var_up"].median().item()
    print(f"  {cid}: median variance entering norm4 of layer 0 {v4:.2e}, entering the upscaler's LayerNorm2d {vu:.2e}")
    assert 1e-5 <= v4 <= 1e-3 and 1e-5 <= vu <= 1e-3
    a = R.refs("A")[0]
    assert a["_var4.0"].median().item() > 0.1 and a["_var_up"].median().item() > 0.1


@torch.no_grad()
@pytest.mark.parametrize("cid,depth", [(c, 2) for c in R.CPU_CASES] + [(c, 1) for c in ("A", "Bcut", "GA", "G5")])
def test_every_mistake_discriminates_where_it_reaches(cid, depth):
    """dec_depth = 2 on every CPU case; dec_depth = 1 (layer 0 followed directly by the final attention) on A, B's cut, G."""
    ref = R.refs(cid, depth)[0]
    names = R.seam_names(depth)
    for m, first in R.MISTAKES.items():
        share = R.reach(cid, m, depth)
        if share == 0.0:                                   # not reached: a no-op on every seam
            wrong = R.run(cid, F64, depth, m)
            assert all(torch.equal(wrong[s], ref[s]) for s in names), (cid, m)
            print(f"  mistake '{m}': no-op in case {cid}, as its geometry says")
            continue
        wrong = R.run(cid, F64, depth, m, upto=first)
        for s in names[:names.index(first)]:
            assert torch.equal(wrong[s], ref[s]), (cid, m, s)
        bound = R.bound(cid, depth, first)
        if m in EPS_MISTAKES and not R.case(cid)["small"]:
            f = Y.quantiles((wrong[first] - ref[first]).abs()) / bound
            print(f"  mistake '{m}' in case {cid} (variance O(1)): " + " ".join(f"{x:.1f}x" for x in f) + " - not decisive")
            assert not torch.equal(wrong[first], ref[first]) and f.max() < Y.MIN_FACTOR
            continue
        Y.assert_discriminates(wrong[first], ref[first], bound, f"{cid} depth {depth} {first}: {m}", share)


def test_every_mistake_is_reached_by_a_cpu_case():
    for m in R.MISTAKES:
        hits = [cid for cid in R.CPU_CASES if R.reach(cid, m) > 0 and (m not in EPS_MISTAKES or R.case(cid)["small"])]
        assert hits, m
    assert R.reach("A", "layer 1 self-attention without pe", 1) == 0.0


@torch.no_grad()
@pytest.mark.parametrize("cid", R.CPU_CASES)
def test_bound_at_low_stays_fp32_grade(cid):
    """At every quantile the bound at `low` is <= 1/SAM_CAP of the error of the float64 restatement with f16-rounded
    linear operands: an engine path fallen to f16 grade cannot pass."""
    ref = R.refs(cid)[0]
    with S.f16_operands():
        emul = R.run(cid, F64)
    for s in ("low", "iou"):
        eq = Y.quantiles((emul[s] - ref[s]).abs())
        bound = R.bound(cid, 2, s)
        print(f"  {cid} {s}: f16-operand error / bound = " + " ".join(f"{x:.0f}" for x in eq / bound))
        if s == "low":
            assert (Y.SAM_CAP * bound <= eq).all(), (cid, eq.tolist(), bound.tolist())


def test_cases_have_the_geometry_they_claim():
    nt = {cid: R.n_tokens(R.case(cid)) for cid in ("A", "B", "C1", "C3", "C10", "D8", "D11", "E")}
    assert nt == {"A": 7, "B": 7, "C1": 7, "C3": 9, "C10": 16, "D8": 8, "D11": 11, "E": 7}
    b = R.case("B")
    assert len(b["img"]) == 17 and set(b["img"]) == {0, 2, 3} and b["emb"].shape[0] == 4
    assert list(b["img"]) != sorted(b["img"])
    for cid in ("C3", "C10"):
        lab = R.case(cid)["labels"]
        assert (lab[:, 0] == 1).all() and {-1, 0, 1} <= set(lab.flatten().tolist())
    m = R.case("E")["mask_input"]
    assert (m[1] == -8).all() and set(m[2].flatten().tolist()) == {-32.0, 32.0} and m[0].std() > 0.1
    assert torch.equal(m[2, 0, :2, :2], torch.full((2, 2), 32.0)) and (m[2, 0, :2, 2:4] == -32).all()
    cut, f = R.case("Bcut"), R.case("F04")
    assert torch.equal(cut["boxes"], b["boxes"][:3]) and torch.equal(f["boxes"], b["boxes"][:3])
    assert all(torch.equal(cut["emb"][i], b["emb"][j]) for i, j in zip(cut["img"], b["img"][:3]))
    e = R.embeddings(4)                    # no image is near a scaled copy of another
    for i in range(4):
        for j in range(i):
            cos = torch.nn.functional.cosine_similarity(e[i].flatten(), e[j].flatten(), 0).item()
            assert abs(cos) < 0.1


@torch.no_grad()
@pytest.mark.parametrize("cid", ["Bcut", "C10"])
def test_split_operands_alone_stay_inside_the_bound(cid):
    """The float64 restatement with every linear's operands split as the engine's GEMMs split them ([hi | lo * 64 | hi / 64]
    against [W_hi | W_hi / 64 | W_lo * 64], each segment rounded to f16) stays within the yardstick at every seam and
    quantile, in fact below the float32 evaluation's own error at the maximum: the operand split by itself leaves the
    engine 8x of room, so a seam that leaves the bound on the GPU does so for another reason (accumulation, a kernel)."""
    ref, f32 = R.refs(cid)
    with R.split_operands():
        emul = R.run(cid, F64)
    for s in R.seam_names(2):
        eq = Y.quantiles((emul[s] - ref[s]).abs())
        fq = Y.quantiles((f32[s].double() - ref[s]).abs())
        print(f"  {cid} {s}: split-operand error / float32 error = " + " ".join(f"{a / b:.2f}" if b else "-" for a, b in zip(eq, fq)))
        assert (eq <= R.bound(cid, 2, s)).all(), (cid, s, eq.tolist())
        assert ref[s].numel() < R.MIN_POP or eq[-1] <= fq[-1], (cid, s, eq.tolist(), fq.tolist())
