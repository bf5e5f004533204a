"""What a caption costs the detector (development aid; MI355X, one process).

Reports, for 800 x 800 images and random weights (the time does not depend on them):
  * detector forward, ms, at B = 1 and B = 8 for captions of T = 4 (both fusion paths: folded, and unfolded on
    ops.biattn_wide), 17, 64 and 256 tokens - eager, allow_graph=False, so that every T is measured the same way;
  * ops.biattn_wide alone at S = 13294 for the same T, next to its byte floor: QV read twice for q (both passes) and
    once for values_v, out_v written once - 8 KiB per image token - over 8 TB/s.
Every case is warmed up; the cases are then timed in alternation over several rounds with device events, and the
median and the spread (min .. max) of the rounds are printed."""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
HBM_BYTES_PER_S = 8e12
TS = (4, 17, 64, 256)


def caption_ids(T: int):
    """[CLS] w w w . w w w . ... [SEP]: T ids with a separator every fourth token."""
    body = [1012 if i % 4 == 3 else 2000 + i for i in range(T - 2)]
    return [101] + body + [102] if T >= 2 else [101]


def timed(cases, rounds: int, inner: int):
    """{name: callable} -> {name: [ms per call, one per round]}, the cases alternating inside every round."""
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    for fn in cases.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in cases}
    for _ in range(rounds):
        for name, fn in cases.items():
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / inner)
    return out


def show(title, res, floors=None):
    print(title)
    for name, ms in res.items():
        med = statistics.median(ms)
        extra = ""
        if floors and floors.get(name):
            extra = f"   floor {floors[name] * 1e3:7.1f} us = {100 * floors[name] / med:4.1f} % of the time"
        print(f"  {name:44s} {med:8.3f} ms  ({min(ms):.3f} .. {max(ms):.3f}){extra}")


def main(rounds: int = 7) -> None:
    from inklayer_amd import gdino, ops, synthetic, weights_init
    if not torch.cuda.is_available():
        raise SystemExit("caption_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    cfg = gdino.GDinoConfig()
    sd = weights_init.random_gdino_state_dict(cfg, dev)
    hw = (800, 800)
    # ---- the kernel alone
    S, sc = 13294, 256 ** -0.5
    g = torch.Generator(device=dev).manual_seed(0)
    qv = torch.randn((S, 2048), generator=g, device=dev).half()
    kls = {T: torch.randn((T, 2048), generator=g, device=dev).half() for T in TS}
    cases = {f"biattn_wide S={S} T={T}": (lambda T=T: ops.biattn_wide(qv, kls[T], 1, S, T, sc)) for T in TS}
    floor_ms = S * 8192 / HBM_BYTES_PER_S * 1e3
    show(f"bi-attention alone, B = 1 (byte floor: 8 KiB per image token = {floor_ms * 1e3:.1f} us)",
         timed(cases, rounds, 20), {k: floor_ms for k in cases})
    del qv
    # ---- the detector forward
    for B in (1, 8):
        imgs = [torch.from_numpy(synthetic.synthetic_sketch(i, hw[0], hw[1])).to(dev) for i in range(B)]
        engines = {}
        for T in TS:
            for fold in ((True, False) if T == 4 else (False,)):
                eng = gdino.GDinoEngine(sd, cfg, dev, encoded_text=weights_init.random_text_features(cfg, dev, n_tokens=T),
                                        token_ids=caption_ids(T))
                eng.fold_fusion = fold
                name = f"forward B={B} T={T}" + (" (folded)" if T == 4 and fold else " (biattn_wide)" if T == 4 else "")
                engines[name] = eng
        cases = {name: (lambda e=e: e.forward(imgs, allow_graph=False)) for name, e in engines.items()}
        show(f"detector forward, {hw[0]} x {hw[1]}, eager", timed(cases, rounds, 3 if B == 1 else 1))
        del engines, cases
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
