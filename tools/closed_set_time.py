"""What closed-set post-processing costs after the detector's forward (development aid; MI355X, one process).

For logits f32 [B, 900, 256] and boxes [B, 900, 4] already on the device - random numbers; a full caption of T = 256
tokens and the C = 127 one-token classes that fill it ("w . " each, between [CLS] and [SEP]) - at B = 1 and B = 8, the
best 300 (query, class) pairs per image:
  gpu tail    ops.class_scores -> ops.topk_rowmax -> ops.select_boxes -> ONE D2H copy of [B, 300, 6]
              (what GDinoEngine.predict_classes runs after forward)
  host        what a user writes without it, PostProcessCocoGrounding.forward (GD/demo/test_ap_on_coco.py:99-137) on the
              host: ONE D2H copy of cat(logits, boxes) [B, 900, 260], then torch on the CPU (sigmoid, matmul with the
              positive map, topk, gather, cxcywh -> xyxy, scale)
  gpu kernels the three launches alone, without the copy (device events)
Both ends with the results on the host, so both are wall-clock times around a call that synchronises (the D2H copy); the
device is idle before each call.  Every case is warmed up, the cases alternate inside each round, and the median and the
spread (min .. max) over the rounds are printed, with the number of CPU threads torch used."""
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
NQ, T, NUM_SELECT = 900, 256, 300
C = (T - 2) // 2                                     # "w ." per class


def positive_map():
    pm = torch.zeros(C, T)
    for c in range(C):
        pm[c, 1 + 2 * c] = 1.0
    return pm / (pm.sum(-1)[:, None] + 1e-6)


def main(rounds: int = 15, inner: int = 10) -> None:
    from inklayer_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("closed_set_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    pm_host = positive_map()
    pm_dev = pm_host.to(dev)
    print(f"nq = {NQ}, T = {T}, C = {C}, num_select = {NUM_SELECT}; torch CPU threads: {torch.get_num_threads()}")
    for B in (1, 8):
        g = torch.Generator(device=dev).manual_seed(B)
        logits = -3.0 + 2.0 * torch.randn((B, NQ, T), generator=g, device=dev)
        boxes = torch.rand((B, NQ, 4), generator=g, device=dev)
        sizes = torch.tensor([[800.0, 1333.0]] * B)                       # (h, w)
        scale = torch.stack([sizes[:, 1], sizes[:, 0]], dim=1).contiguous().to(dev)

        def kernels():
            prob = ops.class_scores(logits, pm_dev)
            idx, val = ops.topk_rowmax(prob.view(B, NQ * C, 1), NUM_SELECT, want_values=True)
            xyxy, labels, _ = ops.select_boxes(idx, boxes, scale, C)
            return val, labels, xyxy

        def gpu_tail():
            val, labels, xyxy = kernels()
            return torch.cat([val[..., None], labels.float()[..., None], xyxy], dim=-1).cpu()

        def host():
            both = torch.cat([logits, boxes], dim=-1).cpu()
            lg, bx = both[..., :T], both[..., T:]
            prob = lg.sigmoid() @ pm_host.T
            values, indexes = torch.topk(prob.view(B, -1), NUM_SELECT, dim=1)
            q, labels = indexes // C, indexes % C
            cx, cy, w, h = bx.unbind(-1)
            xyxy = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)
            xyxy = torch.gather(xyxy, 1, q.unsqueeze(-1).repeat(1, 1, 4))
            img_h, img_w = sizes.unbind(1)
            return values, labels, xyxy * torch.stack([img_w, img_h, img_w, img_h], dim=1)[:, None, :]

        # the two agree (scores to f32 rounding; the same pairs but for near-ties)
        a, (v, l, x) = gpu_tail(), host()
        same = (a[..., 1].long() == l).float().mean().item()
        print(f"B = {B}: scores differ by at most {(a[..., 0] - v).abs().max().item():.2e}, "
              f"{100 * same:.1f} % of the positions carry the same label")
        cases = {"gpu tail (3 launches + D2H [B,300,6])": gpu_tail, "host (D2H [B,900,260] + torch CPU)": host}
        for fn in cases.values():
            for _ in range(3):
                fn()
        res = {k: [] for k in cases}
        dev_ms = []
        for _ in range(rounds):
            for name, fn in cases.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                res[name].append((time.perf_counter() - t0) * 1e3 / inner)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                kernels()
            e1.record()
            e1.synchronize()
            dev_ms.append(e0.elapsed_time(e1) / inner)
        res["gpu kernels alone (device events)"] = dev_ms
        d2h_tail, d2h_host = B * NUM_SELECT * 6 * 4, B * NQ * (T + 4) * 4
        print(f"  D2H bytes: gpu tail {d2h_tail}, host {d2h_host}")
        for name, ms in res.items():
            print(f"  {name:42s} {statistics.median(ms):8.3f} ms  ({min(ms):.3f} .. {max(ms):.3f})")


if __name__ == "__main__":
    main()
