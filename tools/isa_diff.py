"""Compare the gfx950 device code of two source trees, kernel by kernel.

    python tools/isa_diff.py <tree A> <tree B>

Compiles every inklayer_amd/csrc/*.hip of each tree to device assembly with build.FLAGS, splits it per function, strips
comments and mangled symbol names, and prints for every kernel its instruction count, its resource metadata and whether
the two trees agree.  Compared are a function's text up to its end label (which holds its .amdhsa_kernel block, so
accum_offset and every other directive too) and the metadata fields below.  A kernel that moved to another file is
followed by its name and printed as `old.hip->new.hip:kernel`.  Exits 1 if anything differs.  A refactor
that only moves __forceinline__ code must come out `identical` everywhere; the tool looks for no particular instruction.
"""
from __future__ import annotations

import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from inklayer_amd.build import FLAGS, HIPCC  # noqa: E402

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".kernarg_segment_size")
SYM = re.compile(r"_Z\w+")


def assembly(src: Path, out: Path) -> str:
    r = subprocess.run([HIPCC, *FLAGS, "-w", "--offload-device-only", "-S", str(src), "-o", str(out)],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    return out.read_text()


def kernels(asm: str) -> dict[str, tuple[list[str], dict[str, str]]]:
    """{function name: (normalised lines, metadata)} of one file's assembly."""
    out: dict[str, tuple[list[str], dict[str, str]]] = {}
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end\d+:\n", asm, re.M | re.S):
        lines = []
        for line in m.group(2).splitlines():
            line = SYM.sub("_Z", re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", line.split(";")[0])).strip()
            if line:
                lines.append(line)
        out[m.group(1)] = (lines, {})
    for m in re.finditer(r"^  - (\.\w+:.*?)(?=^  - \.|^amdhsa\.)", asm, re.M | re.S):   # one kernel of amdgpu_metadata
        f = dict(re.findall(r"^    (\.\w+): +(\S+)$", "    " + m.group(1), re.M))
        if f.get(".name") in out:
            out[f[".name"]][1].update({k: f.get(k, "-") for k in META})
    return out


def tree(root: Path, tmp: Path) -> dict[str, tuple[list[str], dict[str, str]]]:
    srcs = sorted((root / "inklayer_amd" / "csrc").glob("*.hip"))
    tmp.mkdir()
    with ThreadPoolExecutor(max_workers=16) as ex:
        texts = list(ex.map(lambda s: assembly(s, tmp / (s.stem + ".s")), srcs))
    return {f"{s.name}:{k}": v for s, t in zip(srcs, texts) for k, v in kernels(t).items()}


def follow_moves(a: dict, b: dict) -> dict[str, str]:
    """A kernel that left its file in A and whose name occurs once in each tree is compared with its namesake in B:
    b is re-keyed in place, and {A's key: B's file} of those kernels is returned."""
    def by_name(t):
        out: dict[str, list[str]] = {}
        for k in t:
            out.setdefault(k.split(":", 1)[1], []).append(k)
        return out
    na, nb = by_name(a), by_name(b)
    moved = {}
    for n, ka in na.items():
        kb = nb.get(n, [])
        if len(ka) == 1 and len(kb) == 1 and ka[0] != kb[0]:
            b[ka[0]] = b.pop(kb[0])
            moved[ka[0]] = kb[0].split(":", 1)[0]
    return moved


def main() -> int:
    with tempfile.TemporaryDirectory() as d:
        a, b = tree(Path(sys.argv[1]), Path(d) / "a"), tree(Path(sys.argv[2]), Path(d) / "b")
    moved = follow_moves(a, b)
    names = subprocess.run(["c++filt", "-p"], input="\n".join(k.split(":", 1)[1] for k in sorted(a.keys() | b.keys())),
                           capture_output=True, text=True).stdout.splitlines()
    bad = 0
    print("file:kernel  instructions  " + " ".join(k[1:] for k in META) + "  verdict")
    for key, name in zip(sorted(a.keys() | b.keys()), names):
        (la, ma), (lb, mb) = a.get(key, ([], {})), b.get(key, ([], {}))
        same = la == lb and ma == mb
        bad += not same
        count = lambda ls: sum(1 for l in ls if not l.startswith(".") and not l.endswith(":"))  # noqa: E731
        for ls, ms, tag in ((la, ma, "identical"),) if same else ((la, ma, "differs: A"), (lb, mb, "differs: B")):
            where = key.split(":")[0] + ("->" + moved[key] if key in moved else "")
            print(f"{where}:{name.replace('(anonymous namespace)::', '')}  {count(ls)}  "
                  + " ".join(ms.get(k, "-") for k in META) + f"  {tag}")
    print(f"{len(names)} kernels, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
