"""SAM point / box / mask prompts and multimask output, CPU side: the float64 restatement (tests/sam_prompt_ref.py)
against the reference's own modules (tests/golden/sam_prompts_small.npz), the prompt validation of
inklayer_amd.sam.check_prompts, the coordinate transform, and argument rejection by the new C exports (no GPU)."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "sam_prompts_small.npz"
SMALL = dict(embed_dim=160, depth=4, num_heads=2, global_attn_indexes=(1, 3), window_size=14, img_size=512,
             prompt_embed_dim=64, dec_depth=2, dec_heads=2, dec_mlp_dim=128, iou_head_hidden=64, mask_in_chans=16)


@pytest.fixture(scope="module")
def small():
    from oracle import sam_ref
    import sam_prompt_ref as R
    z = np.load(GOLDEN)
    cfg = sam_ref.SamConfig(**SMALL)
    sd = R.to64(sam_ref.seeded_state_dict(sam_ref.sam_param_shapes(cfg), int(z["seed"])))
    return z, cfg, sd


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("case", ["pts", "ptsbox", "boxmask"])
def test_restatement_matches_reference(small, case):
    import sam_prompt_ref as R
    z, cfg, sd = small
    get = lambda k: torch.from_numpy(z[f"{case}_{k}"]) if f"{case}_{k}" in z else None
    pts, lab, box, msk = get("points"), get("labels"), get("boxes"), get("masks")
    sparse = R.embed_sparse(sd, cfg, pts, lab, box)
    assert sparse.shape == z[f"{case}_sparse"].shape
    assert _rel(sparse, z[f"{case}_sparse"]) < 1e-5
    if msk is not None:
        assert _rel(R.mask_downscaling(sd, msk)[:, :, ::4, ::4], z[f"{case}_dense_sub"]) < 1e-5
    P = sparse.shape[0]
    emb = torch.from_numpy(z["image_embedding"]).expand(P, -1, -1, -1)
    low, iou = R.decode_all(sd, cfg, emb, sparse, msk)
    assert low.shape[1] == 4 and iou.shape == (P, 4)
    assert _rel(low[:, :, ::4, ::4], z[f"{case}_low_sub"]) < 1e-4
    assert _rel(iou, z[f"{case}_iou"]) < 1e-4


def test_apply_coords_matches_reference(small):
    import sam_prompt_ref as R
    from inklayer_amd import sam
    z = small[0]
    hw = tuple(int(v) for v in z["coords_orig_hw"])
    want = z["coords_applied"]
    tr = sam.ResizeLongestSide(1024)
    assert np.array_equal(tr.apply_coords(z["coords_orig"], hw), want)
    assert np.array_equal(R.apply_coords(z["coords_orig"], hw, 1024), want)
    got_t = tr.apply_coords_torch(torch.from_numpy(z["coords_orig"]), hw)
    assert got_t.dtype == torch.float32
    assert torch.allclose(got_t.double(), torch.from_numpy(want), rtol=1e-6, atol=1e-4)
    boxes = z["coords_orig"][:4].reshape(2, 4)
    assert np.array_equal(tr.apply_boxes(boxes, hw), want[:4].reshape(2, 4))


def test_check_prompts():
    from inklayer_amd.sam import MAX_TOKENS, check_prompts
    f, i = torch.zeros, lambda *s: torch.ones(*s, dtype=torch.int32)
    assert check_prompts(f(1, 3, 2), i(1, 3)) == (1, 9)                      # 3 points + pad
    assert check_prompts(f(2, 10, 2), i(2, 10)) == (2, MAX_TOKENS)           # 10 points + pad
    assert check_prompts(f(2, 9, 2), i(2, 9), f(2, 4)) == (2, MAX_TOKENS)    # box + 9 points
    assert check_prompts(None, None, f(3, 4)) == (3, 7)
    assert check_prompts(None, None, f(3, 4), f(3, 1, 256, 256)) == (3, 7)
    assert check_prompts(None, None, None, f(2, 1, 256, 256)) == (2, 5)
    assert check_prompts(np.zeros((1, 2, 2)), np.array([[1.0, 0.0]])) == (1, 8)    # integer-valued float labels
    bad = [
        ((f(1, 11, 2), i(1, 11)), "limit of 16"),                  # NT = 17
        ((f(1, 10, 2), i(1, 10), f(1, 4)), "limit of 16"),         # NT = 17
        ((f(1, 3, 2), None), "together"),
        ((None, i(1, 3)), "together"),
        ((f(1, 3), i(1, 3)), "point_coords"),
        ((f(1, 3, 2), i(1, 3, 2)), "point_labels"),
        ((f(1, 3, 2), torch.full((1, 3), 0.5)), "point_labels"),
        ((i(1, 3, 2), i(1, 3)), "point_coords"),                   # integer coordinates
        ((None, None, f(2, 5)), "boxes"),
        ((None, None, f(2, 4), f(2, 256, 256)), "mask_input"),
        ((None, None, f(2, 4), f(2, 1, 128, 128)), "mask_input"),
        ((f(2, 3, 2), i(2, 3), f(3, 4)), "batch size"),
        ((None, None, f(0, 4)), "at least one"),
    ]
    for args, msg in bad:
        with pytest.raises(ValueError, match=msg):
            check_prompts(*args)


def test_new_exports_reject_bad_arguments_without_launch():
    from inklayer_amd import build, _lib
    build.build(verbose=False)
    l = _lib.lib()
    p = 16                                                     # a non-null (never dereferenced) pointer
    # ink_sam_prompt_tokens: null output, 17 tokens, pad out of {0, 1}, points without labels
    args = dict(points=p, labels=p, n_pts=3, pad=1, boxes=None, gauss=p, F=128, pe=p, nap=p, out_tok=p, size=1024.0,
                P=2, out=p)
    call = lambda **kw: l.ink_sam_prompt_tokens(*{**args, **kw}.values(), None)
    assert call(out=None) == 1
    assert call(n_pts=11) == 1 and call(n_pts=9, boxes=p) == 1        # NT = 17
    assert call(pad=2) == 1 and call(labels=None) == 1 and call(P=0) == 1 and call(size=0.0) == 1
    # ink_sam_mask_embed: wrong parameter count, grid above 64, misaligned pointers, null emb_rows
    margs = dict(mask=p, emb=p, rows=p, prm=p, n_prm=4684, eps=1e-6, P=1, g=64, keys=p, split=None)
    mcall = lambda **kw: l.ink_sam_mask_embed(*{**margs, **kw}.values(), None)
    assert mcall(n_prm=4683) == 1 and mcall(g=65) == 1 and mcall(keys=20) == 1 and mcall(rows=None) == 1
    assert mcall(split=18) == 1 and mcall(P=0) == 1
    # ink_sam_upscale_tail: mask counts other than 1, 3, 4; bad ld_tok
    uargs = dict(u0=p, ld=512, n=1, g=64, lg=p, lb=p, eps=1e-6, blob=p, b3=p, hyper=p, M=3, low=p)
    ucall = lambda **kw: l.ink_sam_upscale_tail(*{**uargs, **kw}.values(), None)
    assert ucall(M=2) == 1 and ucall(M=5) == 1 and ucall(M=0) == 1 and ucall(ld=100) == 1 and ucall(low=None) == 1
    # ink_attn_fewq (f32 rows): head_dim other than 16, a head count that is no multiple of 4, more than 16 queries
    fargs = dict(Q=p, ldq=128, K=p, ldk=128, V=p, ldv=128, nb=1, nq=9, nk=4096, nh=8, hd=16, scale=0.25, qr=None,
                 kvr=None, kadd=None, O=p, ldo=128)
    fcall = lambda **kw: l.ink_attn_fewq(*{**fargs, **kw}.values(), None)
    assert fcall(hd=32) == 1 and fcall(nh=6) == 1 and fcall(nh=2) == 1 and fcall(nq=17) == 1
    # ink_attn_fewkeys: f16 rows exist for head_dim 32 and 64 only
    kargs = dict(Q=p, ldq=128, K=p, ldk=128, V=p, ldv=128, B=1, nq=7, nk=7, nh=8, hd=16, scale=0.25, blocked=None,
                 qr=None, qadd=None, io=0, O=p, ldo=128)
    assert l.ink_attn_fewkeys(*kargs.values(), None) == 1
