"""What a caption costs the detector (development aid; MI355X, one process).

Reports, for 800 x 800 images and random weights (the time does not depend on them):
  * detector forward, ms, at B = 1 and B = 8 for captions of T = 4 (both fusion paths: folded, and unfolded on
    ops.biattn_wide), 17, 64 and 256 tokens - eager, allow_graph=False, so that every T is measured the same way;
  * ops.biattn_wide alone at S = 13294 for the same T, next to its byte floor: QV read twice for q (both passes) and
    once for values_v, out_v written once - 8 KiB per image token - over 8 TB/s;
  * the mixed batch (one caption per image, GDinoEngine.set_captions), captions of MIXED = 256, 64, 17, 17, 9, 9, 4, 4
    tokens: (a) one B = 8 forward in the per-image form, (b) what a caller without it does - the eight B = 1 forwards,
    one engine per caption so that no set_caption host time is counted, (c) B = 8 with all eight captions at 256
    tokens, and (d) ops.biattn_wide_varlen alone at B = 8, S = 13294 for the mixed lengths against the uniform T = 256
    launch.  `--mixed-only` runs only this part.
Every case is warmed up; the cases are then timed in alternation over several rounds with device events, and the
median and the spread (min .. max) of the rounds are printed."""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
HBM_BYTES_PER_S = 8e12
TS = (4, 17, 64, 256)
MIXED = (256, 64, 17, 17, 9, 9, 4, 4)


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


def mixed_batch(rounds: int, dev, cfg, sd, hw) -> None:
    """The mixed-batch cases (a) - (d) of the module docstring."""
    from inklayer_amd import gdino, ops, synthetic, weights_init
    B, S, sc = len(MIXED), 13294, 256 ** -0.5
    g = torch.Generator(device=dev).manual_seed(1)
    qv = torch.randn((B * S, 2048), generator=g, device=dev).half()
    kl = torch.randn((B * 256, 2048), generator=g, device=dev).half()
    t_len = torch.tensor(MIXED, dtype=torch.int32, device=dev)
    cases = {f"(d) biattn_wide_varlen B={B} S={S} mixed": lambda: ops.biattn_wide_varlen(qv, kl, B, S, 256, t_len, sc),
             f"(d) biattn_wide B={B} S={S} T=256": lambda: ops.biattn_wide(qv, kl, B, S, 256, sc)}
    show(f"bi-attention alone, B = {B}, lengths {MIXED}", timed(cases, rounds, 5))
    del qv, kl, cases
    torch.cuda.empty_cache()
    imgs = [torch.from_numpy(synthetic.synthetic_sketch(i, hw[0], hw[1])).to(dev) for i in range(B)]
    feats = {T: weights_init.random_text_features(cfg, dev, n_tokens=T) for T in set(MIXED)}
    make = lambda T: gdino.GDinoEngine(sd, cfg, dev, encoded_text=feats[T], token_ids=caption_ids(T))   # noqa: E731
    per_image, all_long = make(4), make(4)
    per_image.set_captions([caption_ids(T) for T in MIXED], encoded_texts=[feats[T] for T in MIXED])
    all_long.set_captions([caption_ids(256)] * B, encoded_texts=[feats[256]] * B)      # equal captions: the shared form
    assert per_image.captions is not None and all_long.captions is None and all_long.T == 256
    single = {T: make(T) for T in set(MIXED)}

    def eight_single():
        for im, T in zip(imgs, MIXED):
            single[T].forward([im], allow_graph=False)

    cases = {"(a) forward B=8, one caption per image": lambda: per_image.forward(imgs),
             "(b) eight B=1 forwards, those captions": eight_single,
             "(c) forward B=8, all captions T=256": lambda: all_long.forward(imgs, allow_graph=False)}
    show(f"detector forward, {hw[0]} x {hw[1]}, eager, caption lengths {MIXED}", timed(cases, rounds, 1))


def main(rounds: int = 7, mixed_only: bool = False) -> None:
    from inklayer_amd import gdino, ops, synthetic, weights_init
    if not torch.cuda.is_available():
        raise SystemExit("caption_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    cfg = gdino.GDinoConfig()
    sd = weights_init.random_gdino_state_dict(cfg, dev)
    hw = (800, 800)
    if mixed_only:
        return mixed_batch(rounds, dev, cfg, sd, hw)
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
    mixed_batch(rounds, dev, cfg, sd, hw)


if __name__ == "__main__":
    main(mixed_only="--mixed-only" in sys.argv[1:])
