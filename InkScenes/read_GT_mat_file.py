"""Ground-truth viewer of the InkScenes data set (reference surface: InkScenes/read_GT_mat_file.py), on top of
inklayer_amd.evaluate.label_picture: the same names, arguments and command line, the same picture.

    python InkScenes/read_GT_mat_file.py --mat_file 0001.mat [--type INSTANCE_GT] [--output ./vis_mat.png]

Besides .mat files the path may be anything inklayer_amd.evaluate.load_labels reads (.npy, .png, a directory of
mask_<i>.png)."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from inklayer_amd import evaluate, visualize  # noqa: E402


def generate_pastel_colors(n_colors):
    """n_colors pastel (R, G, B) tuples in the interleaved hue order."""
    return visualize.pastel_colors(n_colors)


def visualize_label_matrix(mat_path, mat_type, out_path):
    """mat_path: the .mat file; mat_type: the matrix in it ("INSTANCE_GT" or "CLASS_GT"); out_path: where the picture
    goes.  Returns the PIL image that was saved."""
    from PIL import Image
    picture = evaluate.label_picture(evaluate.load_labels(mat_path, key=mat_type))
    annotated_sketch = Image.fromarray(picture)
    annotated_sketch.save(out_path)
    return annotated_sketch


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="Paint a ground-truth label matrix, one pastel colour per label")
    parser.add_argument("--mat_file", type=str, required=True, help="ground-truth file (.mat; also .npy, .png, mask directory)")
    parser.add_argument("--type", type=str, default="INSTANCE_GT", help="matrix inside the .mat file: INSTANCE_GT or CLASS_GT")
    parser.add_argument("--output", type=str, default="./vis_mat.png", help="picture to write")
    args = parser.parse_args()
    visualize_label_matrix(args.mat_file, args.type, args.output)
