"""Records what the reference's ground-truth viewer (InkScenes/read_GT_mat_file.py: visualize_label_matrix) paints for five
small label matrices into tests/golden/gtvis_small.npz.

Each matrix is written to a temporary .mat file with scipy.io.savemat under the key INSTANCE_GT, the reference's function
is called on it, and only the resulting pixels are stored next to the matrix itself:
  labels_<k>    the matrix as it was handed to savemat
  picture_<k>   uint8 [H, W, 3]: the PNG the reference wrote, read back
  names         what each matrix is

    python tests/golden/make_gtvis_golden.py        # build container only (/root/reference; needs scipy, matplotlib)
"""
import importlib.util
import io
import tempfile
from pathlib import Path

import numpy as np
from PIL import Image
from scipy.io import savemat

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
H, W = 40, 56


def matrices():
    rs = np.random.RandomState(27)

    def blocks(values, dtype):
        """A coarse random layout (8 x 8 blocks) of the given values with a few single pixels on top."""
        values = np.asarray(values)
        coarse = values[rs.randint(0, len(values), size=(H // 8, W // 8))]
        lab = np.kron(coarse, np.ones((8, 8), coarse.dtype))
        spots = rs.rand(H, W) < 0.05
        lab[spots] = values[rs.randint(0, len(values), size=int(spots.sum()))]
        lab.reshape(-1)[:len(values)] = values                    # every value occurs
        return lab.astype(dtype)

    return [("uint8 with background: 0, 1, 2, 5, 9", blocks([0, 1, 2, 5, 9], np.uint8)),
            ("no background: 3, 4, 7", blocks([3, 4, 7], np.uint8)),
            ("uint16 up to 60000", blocks([0, 17, 300, 4096, 59999, 60000], np.uint16)),
            ("float64 as loadmat may return it", blocks([0, 1, 2, 3, 11, 12, 40], np.float64)),
            ("all zeros", np.zeros((H, W), np.uint8))]


def main():
    spec = importlib.util.spec_from_file_location("_ref_read_gt", REF / "InkScenes/read_GT_mat_file.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    names = []
    with tempfile.TemporaryDirectory() as tmp:
        for k, (name, lab) in enumerate(matrices()):
            mat, png = Path(tmp) / f"m{k}.mat", Path(tmp) / f"m{k}.png"
            savemat(mat, {"INSTANCE_GT": lab})
            mod.visualize_label_matrix(str(mat), "INSTANCE_GT", str(png))
            out[f"labels_{k}"] = lab
            out[f"picture_{k}"] = np.asarray(Image.open(png).convert("RGB"))
            names.append(name)
    out["names"] = np.asarray(names)
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    (OUT / "gtvis_small.npz").write_bytes(buf.getvalue())
    print("gtvis_small.npz", len(buf.getvalue()) >> 10, "KiB")


if __name__ == "__main__":
    main()
