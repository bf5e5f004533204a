"""What the text features of fresh captions cost (development aid; MI355X, one process).

For a random BERT-base (12 layers, vocabulary 30522, weights_init.random_bert_state_dict - the time does not depend on
the values) and B = 1 and 8 DISTINCT captions of T = 4, 23 and 256 tokens it times
  host   the fold GDinoEngine used before the GPU encoder: text_branch.encode_caption_from_checkpoint per caption, one
         after the other, f32 torch on 16 CPU threads - a host clock around the B calls;
  gpu    BertTextEncoder.encode on all B captions at once - a host clock from the call to the end of a device
         synchronise, so the uploads of the ids, masks and row tables are inside; `+copy` adds the B device-to-host
         copies the engine's caption cache keeps.
Each figure is the median of RUNS timed calls after warm-up calls of the same shape, min .. max next to it.  It also
reports the encoder's native launches per pass (counted, not assumed) and its device bytes."""
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
RUNS, WARMUP, THREADS = 11, 2, 16
BS, TS = (1, 8), (4, 23, 256)


def caption_ids(T: int, b: int):
    """[CLS] w w w . w w w . ... [SEP]: T ids with a separator every fourth token; b makes the captions distinct."""
    body = [1012 if i % 4 == 3 else 2000 + 300 * b + i for i in range(T - 2)]
    return tuple([101] + body + [102]) if T >= 2 else (101,)


def clocked(fn, runs=RUNS, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main() -> None:
    from inklayer_amd import ops, text_branch, weights_init
    from inklayer_amd.text_encoder import BertTextEncoder
    if not torch.cuda.is_available():
        raise SystemExit("text_encoder_time.py measures on the GPU: no device found")
    torch.set_num_threads(THREADS)
    dev = torch.device("cuda:0")
    sd = weights_init.random_bert_state_dict(n_layers=12, vocab_size=30522, seed=0)
    t0 = time.perf_counter()
    enc = BertTextEncoder(sd, dev)
    torch.cuda.synchronize()
    print(f"encoder built in {time.perf_counter() - t0:.2f} s, {enc.nbytes / 2 ** 20:.0f} MiB on the device, "
          f"{enc.n_layers} layers; host fold on {torch.get_num_threads()} threads")

    launches, real = [0], ops.check

    def counting(rc, what):
        launches[0] += 1
        return real(rc, what)

    ops.check = counting
    enc.encode([caption_ids(23, 0)])
    ops.check = real
    print(f"native launches per pass: {launches[0]} (launches_per_pass = {enc.launches_per_pass})")

    print(f"{'B':>2} {'T':>4} | {'host fold ms':>28} | {'gpu encode ms':>28} | {'gpu + copies ms':>28} | host / gpu")
    for B in BS:
        for T in TS:
            caps = [caption_ids(T, b) for b in range(B)]

            def host():
                for c in caps:
                    text_branch.encode_caption_from_checkpoint(sd, c)

            def gpu():
                enc.encode(caps)
                torch.cuda.synchronize()

            def gpu_copy():
                return [f.to("cpu", torch.float32) for f in enc.encode(caps)]

            g, gc, h = clocked(gpu), clocked(gpu_copy), clocked(host)
            fmt = lambda r: f"{r[0]:9.3f} ({r[1]:.3f} .. {r[2]:.3f})"      # noqa: E731
            print(f"{B:>2} {T:>4} | {fmt(h):>28} | {fmt(g):>28} | {fmt(gc):>28} | {h[0] / g[0]:8.1f}x", flush=True)


if __name__ == "__main__":
    main()
