"""Detector alone at batch 8 (800x800): wall per forward, and kernel-level stage split with HIP events (development aid).

--model swin_b: the Swin-B/384 backbone instead (random weights, depths (2, 2, 18, 2)): ms per batch of 8, and per stage
the time of the window-attention kernel (ops.swin_attn, shifted and unshifted) with its share of the HBM floor - the
bytes of q, k, v, o moved once, computed from the shapes, over 8 TB/s - next to ops.flash_attn bias_mode 3 at Swin-T
stage 0 and its share of its own floor.  All kernels are warmed up, then timed in alternation over several rounds
with device events; the median and the spread (min .. max) of the rounds are printed."""
import statistics
import sys, time
from pathlib import Path
import torch
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
HBM_BYTES_PER_S = 8e12


def swin_b_report(model: str, B: int = 8, hw=(800, 800), rounds: int = 9, inner: int = 20) -> None:
    from inklayer_amd import gdino, ops, synthetic, weights_init
    dev = torch.device("cuda:0")
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    cfg = gdino.config_for(model)
    eng = gdino.GDinoEngine(weights_init.random_gdino_state_dict(cfg, dev), cfg, dev,
                            encoded_text=weights_init.random_text_features(cfg, dev))
    imgs = [torch.from_numpy(synthetic.synthetic_sketch(i, hw[0], hw[1])).to(dev) for i in range(B)]
    pl = eng.plan(hw[0], hw[1], B)
    ws, scale = cfg.window_size, gdino.HEAD_DIM ** -0.5
    g = torch.Generator(device=dev).manual_seed(0)
    cases = {}                      # name -> (callable, floor in us)
    for i, nh in enumerate(cfg.num_heads):
        C, rows = 32 * nh, B * pl.nW[i] * ws * ws
        qkv = torch.randn((rows, 3 * C), generator=g, device=dev).half()
        out = torch.empty((rows, C), device=dev, dtype=torch.float16)
        floor = 4 * rows * C * 2 / HBM_BYTES_PER_S * 1e6
        for shifted in (0, 1):
            if ws == 7:
                bias = eng.w[f"s{i}b{shifted}.bias"]
                fn = (lambda qkv=qkv, C=C, i=i, nh=nh, bias=bias, out=out, shifted=shifted: ops.flash_attn(
                    qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], n_batch=B * pl.nW[i], n_heads=nh, head_dim=32, scale=scale,
                    n_q=49, n_k=49, dense_bias=bias, dense_mask=pl.shift_mask[i] if shifted else None, out=out))
            else:
                tab = eng.w[f"s{i}b{shifted}.table"]
                fn = (lambda qkv=qkv, C=C, i=i, nh=nh, tab=tab, out=out, shifted=shifted: ops.swin_attn(
                    qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], n_windows=B * pl.nW[i], n_heads=nh, ws=ws, scale=scale,
                    bias_table=tab, region=pl.region[i] if shifted else None, nW=pl.nW[i], out=out))
            cases[f"{model} stage {i} {'shifted' if shifted else 'plain  '} ({rows} rows x {nh} heads)"] = (fn, floor)
    # the comparison: bias_mode 3 at Swin-T stage 0 (7 x 7 windows, 3 heads), dense tables as the Swin-T engine has them
    tcfg = gdino.GDinoConfig()
    tplan = gdino._Plan(type("E", (), dict(cfg=tcfg, dev=dev, level_embed_cpu=torch.zeros(4, 256)))(), hw[0], hw[1], B)
    rows, C = B * tplan.nW[0] * 49, 96
    tq = torch.randn((rows, 3 * C), generator=g, device=dev).half()
    tout = torch.empty((rows, C), device=dev, dtype=torch.float16)
    tbias = gdino.swin_dense_bias(torch.randn(169, 3), 7, 3, scale).to(dev).contiguous()
    for shifted in (0, 1):
        fn = (lambda shifted=shifted: ops.flash_attn(
            tq[:, :C], tq[:, C:2 * C], tq[:, 2 * C:], n_batch=B * tplan.nW[0], n_heads=3, head_dim=32, scale=scale, n_q=49,
            n_k=49, dense_bias=tbias, dense_mask=tplan.shift_mask[0] if shifted else None, out=tout))
        cases[f"swin_t mode 3 stage 0 {'shifted' if shifted else 'plain  '} ({rows} rows x 3 heads)"] = (
            fn, 4 * rows * C * 2 / HBM_BYTES_PER_S * 1e6)
    cases["backbone"] = (lambda: eng.backbone(imgs, pl), None)
    for fn, _ in cases.values():                     # warm up every shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(rounds):                          # alternate: one timed burst of each per round
        for k, (fn, _) in cases.items():
            n = 3 if k == "backbone" else inner
            a, b = ev(), ev()
            a.record()
            for _ in range(n):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / n * 1e3)     # us
    print(f"{model}: B = {B}, {hw[0]} x {hw[1]}, {rounds} alternating rounds, median (min .. max)")
    for k, (_, floor) in cases.items():
        t = times[k]
        med = statistics.median(t)
        if floor is None:
            print(f"  {k:58s} {med / 1e3:8.2f} ms ({min(t) / 1e3:.2f} .. {max(t) / 1e3:.2f}) per batch of {B}")
        else:
            print(f"  {k:58s} {med:8.1f} us ({min(t):.1f} .. {max(t):.1f}); HBM floor {floor:6.1f} us; share "
                  f"{100 * floor / med:5.1f} % ({100 * floor / max(t):.1f} .. {100 * floor / min(t):.1f})")


if len(sys.argv) > 1:
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--model", default=None, help="swin_b (or another registry name): time that backbone and its attention")
    args = ap.parse_args()
    if args.model is not None:
        swin_b_report(args.model)
        sys.exit(0)
import bench
from inklayer_amd import ops, pipeline, synthetic
dev = torch.device("cuda:0")
det, seg, _ = bench.build_engines(dev, 0, 1, 8)
pipe = pipeline.InkLayerPipeline(det, seg, overlap=False)
imgs = [synthetic.synthetic_sketch(i) for i in range(8)]
d, s, z = pipe.prepare(imgs)
for _ in range(2):
    det.forward(d, allow_graph=False)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(5):
    det.forward(d, allow_graph=False)
torch.cuda.synchronize()
print(f"detector forward B=8: {(time.perf_counter() - t0) / 5 * 1e3:.2f} ms wall")
# stage split
pl = det.plan(800, 800, 8)
ev = lambda: torch.cuda.Event(enable_timing=True)
marks = [ev() for _ in range(5)]
marks[0].record(); feats = det.backbone(d, pl)
marks[1].record(); src = det.neck(feats, pl, 8)
marks[2].record(); memory, text = det.encoder(src, pl, 8)
marks[3].record(); det.decoder(memory, text, pl, 8, None)
marks[4].record(); torch.cuda.synchronize()
for n, a, b in zip(("swin backbone", "input_proj+GN", "encoder x6", "two-stage + decoder x6"), marks[:-1], marks[1:]):
    print(f"  {n:26s} {a.elapsed_time(b):7.2f} ms")
t0 = time.perf_counter()
for _ in range(5):
    seg.encode(s, chan_reverse=True)
torch.cuda.synchronize()
print(f"SAM encoder B=8: {(time.perf_counter() - t0) / 5 * 1e3:.2f} ms wall")
