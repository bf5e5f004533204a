"""CPU-side checks of the C-ABI boundary: the library builds, loads and exports every
symbol that include/inklayer_hip.h declares (no compute calls: there is no GPU here)."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _declared_symbols():
    txt = (ROOT / "include" / "inklayer_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\bint\s+(ink_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from inklayer_amd import build, _lib
    build.build(verbose=False)
    import torch  # noqa: F401  torch's HIP runtime first: see inklayer_amd/_lib.py lib()
    l = ctypes.CDLL(str(_lib.lib_path()))
    syms = _declared_symbols()
    assert len(syms) >= 4
    for s in syms:
        assert hasattr(l, s), f"{s} declared in inklayer_hip.h but not exported"
    hdr = (ROOT / "include" / "inklayer_hip.h").read_text()
    assert l.ink_abi_version() == int(re.search(r"#define\s+INK_ABI_VERSION\s+(\d+)", hdr).group(1))


def test_python_binding_covers_header():
    from inklayer_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared_symbols()


def test_bad_arguments_are_rejected_without_launch():
    # argument validation happens before any HIP call, so it is testable without a GPU
    from inklayer_amd import _lib
    l = _lib.lib()
    p = _lib.InkGemm()
    assert l.ink_gemm_f16(ctypes.byref(p), None) == 1          # null pointers
    p.A = p.W = p.C = 16
    p.M, p.N, p.K = 8, 8, 24                                    # K % 32 != 0
    p.lda = p.ldw = 24
    p.ldc = 8
    assert l.ink_gemm_f16(ctypes.byref(p), None) == 1
    p.K = p.lda = p.ldw = 32                                    # well-formed but for the output type: 0 (f32) / 1 (f16) only
    p.c_f16 = 2
    assert l.ink_gemm_f16(ctypes.byref(p), None) == 1
    assert l.ink_layernorm_rows(None, 0, None, None, 1e-6, None, 1, 4, None, None, 4, 0, 0, None, 0, None, 0, None) == 1
    assert l.ink_add_split_f16(16, None, 0, 16, 8, 3, None) == 1            # C % 4 != 0


def test_attn_fewkeys_argument_contract():
    """ink_attn_fewkeys returns 1 before any launch for every form it has no kernel for and for rows or pointers its
    16-byte vector loads and stores cannot take.  Fake non-null pointers: none of these calls may be accepted."""
    from inklayer_amd import _lib
    l = _lib.lib()
    p = 16
    args = dict(Q=p, ldq=128, K=p, ldk=128, V=p, ldv=128, B=1, nq=7, nk=7, nh=8, hd=16, scale=0.25, blocked=None,
                qr=None, qadd=None, io=1, O=p, ldo=128)
    call = lambda **kw: l.ink_attn_fewkeys(*{**args, **kw}.values(), None)
    assert call(nk=17) == 1 and call(nk=0) == 1
    assert call(hd=16, io=0) == 1                       # f16 rows: head_dim 32 and 64 only
    assert call(hd=48) == 1 and call(hd=48, io=0) == 1 and call(hd=64) == 1      # f32 rows: 16 and 32 only
    assert call(io=2) == 1 and call(io=-1) == 1
    assert call(ldq=12) == 1 and call(ldk=132) == 1 and call(ldv=4) == 1 and call(ldo=129) == 1
    assert call(Q=8) == 1 and call(K=24) == 1 and call(V=20) == 1 and call(O=40) == 1
    assert call(qadd=24) == 1 and call(qadd=4) == 1
    assert call(Q=None) == 1 and call(O=None) == 1


def test_attn_fewq_argument_contract():
    """The same for ink_attn_fewq: f32 rows, head_dim 16, n_heads % 4 == 0, n_q <= 16, aligned rows and pointers."""
    from inklayer_amd import _lib
    l = _lib.lib()
    p = 16
    args = dict(Q=p, ldq=128, K=p, ldk=128, V=p, ldv=128, nb=1, nq=9, nk=4096, nh=8, hd=16, scale=0.25, qr=None,
                kvr=None, kadd=None, O=p, ldo=128)
    call = lambda **kw: l.ink_attn_fewq(*{**args, **kw}.values(), None)
    assert call(nq=17) == 1 and call(nq=0) == 1 and call(nk=0) == 1
    assert call(hd=32) == 1 and call(nh=6) == 1
    assert call(ldk=4) == 1 and call(ldq=12) == 1 and call(ldv=130) == 1 and call(ldo=60) == 1
    assert call(K=24) == 1 and call(Q=8) == 1 and call(V=4) == 1 and call(O=72) == 1
    assert call(kadd=24) == 1 and call(kadd=8) == 1
    assert call(K=None) == 1


def test_refine_stage_argument_contract():
    """The ten entry points of csrc/refine_stage.hip return 1 before any launch for: each required pointer null in
    turn, H or W of 0, H or W of 16384 where the entry point launches a word grid computed in int or packs run ends into
    16 bits, 255 ranks, an in-place label image, a cap of 0, P or Q of 0, A < 0.  Fake non-null pointers: none of these
    calls may be accepted.  (Looked up by name from a table, so these calls do not count as tests of the kernels for
    tests/test_op_coverage_cpu.py.)"""
    from inklayer_amd import _lib
    l = _lib.lib()
    size0 = [dict(H=0), dict(W=0)]
    size = size0 + [dict(H=16384), dict(W=16384)]
    null = lambda *names: [{n: None} for n in names]
    table = {
        "ink_refine_sketch_planes": (dict(rgb=16, H=8, W=8, planes=32, max_ws=48),
                                     null("rgb", "planes", "max_ws") + size),
        "ink_bitplane_pack": (dict(img=16, n=2, H=8, W=8, thresh=0, planes=32),
                              null("img", "planes") + size + [dict(n=0), dict(n=-1)]),
        "ink_refine_depth_samples": (dict(planes=16, n=3, depth=32, pts=48, P=5, H=8, W=8, vals=64, inside=80),
                                     null("planes", "depth", "pts", "vals", "inside") + size0
                                     + [dict(P=0), dict(P=-1), dict(n=-1), dict(n=0, depth=None), dict(n=0, vals=None)]),
        "ink_refine_pair_tables": (dict(planes=16, sk=32, n=2, H=8, W=8, rect=48, dil=64, pair=80, per=96, area=112),
                                   null("planes", "sk", "rect", "dil", "pair", "per", "area") + size
                                   + [dict(n=-1), dict(n=0, sk=None), dict(n=0, area=None)]),
        "ink_refine_composite": (dict(planes=16, order=32, nr=3, H=8, W=8, label=48, hist=64),
                                 null("planes", "order", "label", "hist") + size
                                 + [dict(nr=255), dict(nr=-1), dict(nr=0, label=None), dict(nr=0, hist=None)]),
        "ink_refine_relabel_clean": (dict(label=16, lut=32, H=8, W=8, out=48),
                                     null("label", "lut", "out") + size0 + [dict(out=16)]),
        "ink_refine_grow": (dict(label=16, sk=32, H=8, W=8, pws=48, ccw=64, flags=80, out=96, bbox=112, unl=128, cap=4,
                                 count=144),
                            null("label", "sk", "pws", "ccw", "flags", "out", "bbox", "unl", "count") + size
                            + [dict(cap=0), dict(cap=-1), dict(out=16)]),
        "ink_refine_query_dists": (dict(label=16, q=32, cand=48, Q=3, H=8, W=8, d2=64),
                                   null("label", "q", "cand", "d2") + size0 + [dict(Q=0), dict(Q=-1)]),
        "ink_refine_finalize": (dict(label=16, assign=32, A=2, sk=48, H=8, W=8, ws=64, extra=80, count=96),
                                null("label", "assign", "sk", "ws", "extra", "count") + size
                                + [dict(A=-1), dict(A=0, label=None), dict(A=0, extra=None)]),
    }
    for name, (args, bad) in table.items():
        fn = getattr(l, name)
        for kw in bad:
            assert set(kw) <= set(args), (name, kw)
            assert fn(*{**args, **kw}.values(), None) == 1, (name, kw)
    pw, ci = ctypes.c_int64(-1), ctypes.c_int64(-1)
    ws = getattr(l, "ink_refine_grow_workspace")
    assert ws(0, 8, ctypes.byref(pw), ctypes.byref(ci)) == 1 and ws(8, 0, ctypes.byref(pw), ctypes.byref(ci)) == 1
    assert ws(8, 8, None, ctypes.byref(ci)) == 1 and ws(8, 8, ctypes.byref(pw), None) == 1
    assert ws(7, 129, ctypes.byref(pw), ctypes.byref(ci)) == 0 and pw.value == 4 * 7 * 3 and ci.value > 7 * 7 * 65


def _misaligned_cases():
    """name -> (well-formed arguments with fake pointers, {pointer argument: the alignment its entry point demands})
    for the entry points whose pointer checks go through ink_aligned (csrc/common.h) and that no other test module
    feeds a misaligned pointer.  Not here: ink_mask_cleanup (tests/test_mask_handoff_ops_gpu.py feeds it a misaligned
    scratch image), and, because the check cannot fail a call before a launch, the alignment tests of
    msda.hip, visualize.hip, ink_sam_postprocess and ink_eval_*'s vector paths, which choose a kernel, not an error
    (tests/test_visualize_gpu.py, tests/test_evaluate_gpu.py feed those misaligned buffers)."""
    p = 4096
    return {
        "ink_proj256_ln_pack": (dict(ws=p, blob=p), dict(ws=16, blob=16)),
        "ink_proj256_ln": (dict(a=p, blob=p, bias=p, res=p, rbr=None, rpb=0, g=p, b=p, eps=1e-6, rows=128, out=p, split=p),
                           dict(a=16, blob=16, res=16, out=16, split=16)),
        "ink_ffn256_pack": (dict(w1=p, b1=p, w2=p, hid=2048, wpre=p, blob=p), dict(w1=16, wpre=16, blob=16)),
        "ink_ffn256_fused": (dict(x=p, ldx=256, res=p, blob=p, b2=p, g=p, b=p, eps=1e-5, M=128, hid=2048, pb=p, pg=p,
                                  pbe=p, out=p),
                             dict(x=16, res=16, blob=16, b2=16, g=16, b=16, pb=16, pg=16, pbe=16, out=16)),
        "ink_sam_upscale_pack": (dict(ws=p, blob=p), dict(ws=16, blob=16)),
        "ink_sam_upscale_tail": (dict(u0=p, ld=512, n=1, g=64, lg=p, lb=p, eps=1e-6, blob=p, b3=p, hyper=p, M=3, low=p),
                                 dict(u0=16, blob=16, hyper=16, low=16)),
        "ink_conv3x3_f16": (dict(x=p, B=1, H=4, W=4, C=64, w=p, N=8, bias=p, stride=1, relu_in=0, act=0, res=p, out=p,
                                 f16=0),
                            dict(x=16, w=16, bias=16, res=16, out=16)),
        "ink_sam_mask_embed": (dict(mask=p, emb=p, rows=p, prm=p, n_prm=4684, eps=1e-6, P=1, g=64, keys=p, split=p),
                               dict(mask=16, emb=16, keys=16, split=8)),
        "ink_relpos_bias64_f16": (dict(Q=p, ldq=3840, rh=p, rw=p, nb=1, nh=1, hd=80, scale=0.1, oh=p, ow=p),
                                  dict(oh=16, ow=16)),
        "ink_sam_amg_stats": (dict(low=p, n=1, index=None, m=1, m_dev=None, S=256, L=1024, in_h=768, in_w=1024,
                                   crop_h=600, crop_w=800, thr=0.0, off=1.0, x0=0, y0=0, oh=600, ow=800, table=p,
                                   planes=p, logits=p),
                              dict(planes=8, logits=16)),           # crop_w % 4 == 0: the row kernel's 16-byte logits
        "ink_mask_rle_counts": (dict(planes=p, sel=None, k=1, H=600, W=800, n=p), dict(planes=8)),
        "ink_mask_rle_write": (dict(planes=p, sel=None, k=1, H=600, W=800, offs=p, counts=p), dict(planes=8)),
        "ink_box_nms": (dict(boxes=p, scores=p, n=4, iou=0.7, ws=p, keep=p, n_keep=p), dict(ws=16)),
        "ink_mask_small_regions": (dict(planes=p, k=1, H=600, W=800, area=100, holes=1, tmp=p, ws=p, out=p, changed=p),
                                   dict(planes=8, tmp=8, ws=8, out=8)),
        "ink_eval_label_ranks": (dict(lab=p, es=1, H=8, W=8, ws=p, vals=p, cap=256, info=p, rank=p), dict(rank=2)),
        "ink_eval_contingency": (dict(pred=p, n=2, by_label=0, rank=p, U=3, sk=p, ch=3, so=1, H=8, W=8, T=p),
                                 dict(rank=2)),
        "ink_eval_label_boxes": (dict(rank=p, U=3, H=8, W=8, boxes=p), dict(rank=2)),
        "ink_eval_paint_labels": (dict(rank=p, col=p, U=3, H=8, W=8, out=p), dict(rank=2)),
    }


def test_misaligned_pointers_are_refused_without_launch():
    """Every pointer that an entry point's alignment check names, offset by HALF the demanded alignment while every
    other argument is valid, makes the call return 1 before any HIP call.  Fake non-null pointers: none of these calls
    may be accepted.  (Looked up by name from a table, as in test_refine_stage_argument_contract.)"""
    from inklayer_amd import _lib
    l = _lib.lib()
    for name, (args, ptrs) in _misaligned_cases().items():
        fn = getattr(l, name)
        for arg, align in ptrs.items():
            assert args[arg] % align == 0 and align >= 2
            assert fn(*{**args, arg: args[arg] + align // 2}.values(), None) == 1, (name, arg)
    # ink_flash_attn takes a struct: q, k, v rows in 16-byte, o rows in 8-byte pieces; the window form's pad rows
    def attn(**kw):
        a = _lib.InkAttn()
        a.Q = a.K = a.V = a.O = 4096
        a.ldq = a.ldk = a.ldv = 3 * 96 + 8
        a.ldo = 96
        a.n_batch, a.n_heads, a.n_q, a.n_k, a.head_dim, a.scale = 2, 3, 49, 49, 32, 0.25
        for k, v in kw.items():
            setattr(a, k, v)
        return l.ink_flash_attn(ctypes.byref(a), None)
    assert attn(Q=4104) == 1 and attn(K=4104) == 1 and attn(V=4104) == 1 and attn(O=4100) == 1
    win = dict(head_dim=80, bias_mode=2, rel_aug=4096, grid_w=14, n_q=196, n_k=196, ldq=3840, ldk=3840, ldv=3840,
               ldo=1280, tok_rows=4096, pad_k=4096, pad_v=4096)
    assert attn(**{**win, "pad_k": 4104}) == 1 and attn(**{**win, "pad_v": 4104}) == 1


def test_attn_few_wrappers_refuse_misaligned_rows():
    """ops.attn_fewkeys / ops.attn_fewq assert 16-byte aligned q, k, v before anything native is called (CPU tensors: a
    view that starts 8 bytes into a row)."""
    import pytest
    import torch
    from inklayer_amd import ops
    for dtype, col in ((torch.float32, 2), (torch.float16, 4)):
        good = torch.zeros(14, 256, dtype=dtype)
        bad = torch.zeros(14, 272, dtype=dtype)[:, col:col + 256]
        assert good.data_ptr() % 16 == 0 and bad.data_ptr() % 16 == 8 and bad.stride(1) == 1
        for i in range(3):
            qkv = [good, good, good]
            qkv[i] = bad
            with pytest.raises(AssertionError):
                ops.attn_fewkeys(*qkv, B=2, n_heads=8, head_dim=32, scale=0.25)
            if dtype == torch.float32:
                with pytest.raises(AssertionError):
                    ops.attn_fewq(*qkv, n_batch=2, n_heads=16, head_dim=16, scale=0.25, n_q=7, n_k=7)


def test_gemm_variant_hook_accepts_only_shipped_tile_families():
    """VERDICT r1 / ADVICE: the library ships only the GEMM tile families the shape heuristic dispatches, and the test
    hook ink_gemm_set_variant accepts exactly those (-1 = the heuristic): no sweep tiling, no persistent or
    residual-through-MFMA form, no A/B encoding, no ablation kernel.  No environment variable may select a GEMM variant,
    and no kernel source carries a compile-time experiment switch (no preprocessor conditional at all)."""
    from inklayer_amd import _lib
    lib = _lib.lib()
    shipped = {-1, 0, 10, 45}
    removed = (11, 12, 14, 16, 32, 40, 42, 47, 53, 54, 55, 445, 454, 455, -2, 10045)
    ablation = (21, 22, 23, 43, 44, 46, 48, 49, 50, 51, 52, 61, 62, 63)
    try:
        for v in (*removed, *ablation, *range(-4, 1000), 10000, 10010, 10445):
            assert lib.ink_gemm_set_variant(v) == (0 if v in shipped else 1), v
    finally:
        lib.ink_gemm_set_variant(-1)
    src = (ROOT / "inklayer_amd" / "csrc" / "gemm.hip").read_text()
    assert "getenv" not in src
    for f in sorted((ROOT / "inklayer_amd" / "csrc").iterdir()):
        cond = [ln for ln in f.read_text().splitlines() if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", ln)]
        assert not cond, (f.name, cond)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from inklayer_amd import _lib
    monkeypatch.setenv("INKLAYER_HIP_LIB", str(tmp_path / "nope.so"))
    monkeypatch.setattr(_lib, "_lib", None)
    import pytest
    with pytest.raises(_lib.InkLayerHipError):
        _lib.lib()


def test_graft_entry_build_checks_pass():
    """The driver's build hook: (incremental) hipcc build, ABI version of the .so == the header's, imports."""
    import __graft_entry__ as g
    g.build()
