"""Shared inputs of the visualisation tests: the reference's own pictures (tests/golden/vis_<set>.npz next to the inputs
and masks of refine_<set>.npz) and small synthetic sketches."""
from functools import lru_cache
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
SETS = ["Clipasso_brushpen_0249", "animal_hike_sketch", "clock_lamp_plant", "fscoco_animals", "mario_bunny", "office_sketch"]


@lru_cache(maxsize=None)
def load_set(name):
    """-> dict: input uint8 [H, W, 3]; masks / masks_final bool [n, H, W]; the four pictures as the reference saved
    them; the numbers of bboxes.json / bboxes_final.json.  Loaded once per session; treat as read-only."""
    r = np.load(GOLDEN / f"refine_{name}.npz")
    v = dict(np.load(GOLDEN / f"vis_{name}.npz"))
    extra = GOLDEN / f"vis_{name}_boxes.npz"
    if extra.exists():
        v.update(np.load(extra))
    inp = r["input"]
    W = inp.shape[1]
    out = {"input": inp}
    for stage, count in (("masks", "n_masks"), ("masks_final", "n_masks_final")):
        n = int(v[count])
        assert r[stage + "_present"][:n].all() and not r[stage + "_present"][n:].any()
        out[stage] = np.unpackbits(r[stage][:n], axis=-1)[..., :W].astype(bool)
    for key, pic in (("seg_xor", "segmented_sketch"), ("seg_final_xor", "segmented_sketch_final"),
                     ("bboxes_xor", "bboxes_png"), ("bboxes_final_xor", "bboxes_final_png")):
        out[pic] = v[key] ^ inp
    for key in ("bboxes", "scores", "final_bboxes", "final_scores"):
        out[key] = v[key]
    for a in out.values():
        a.setflags(write=False)
    return out


def strokes(rs, H, W, lo=0, hi=250, density=0.35):
    """A grey sketch uint8 [H, W]: white (250 .. 255) with stroke pixels of grey lo .. hi - 1."""
    g = rs.randint(250, 256, size=(H, W))
    on = rs.rand(H, W) < density
    g[on] = rs.randint(lo, hi, size=int(on.sum()))
    return g.astype(np.uint8)


def random_masks(rs, n, H, W, dtype=bool):
    """n overlapping masks: random rectangles with random holes."""
    out = np.zeros((n, H, W), bool)
    for k in range(n):
        y0, x0 = rs.randint(0, H), rs.randint(0, W)
        y1, x1 = rs.randint(y0, H) + 1, rs.randint(x0, W) + 1
        out[k, y0:y1, x0:x1] = rs.rand(y1 - y0, x1 - x0) < 0.8
    return out if dtype is bool else out.astype(dtype)


def rgb_of(gray):
    return np.repeat(np.asarray(gray)[..., None], 3, axis=2)


def synthetic_cases():
    """(name, sketch, list of masks, keyword arguments) at <= 48 x 48: every branch of color_sketch_by_masks."""
    rs = np.random.RandomState(7)
    H, W = 41, 37
    g = strokes(rs, H, W)
    m3 = list(random_masks(rs, 3, H, W))
    cases = [("no stroke pixel at all", rgb_of(rs.randint(250, 256, size=(H, W)).astype(np.uint8)), m3, {}),
             ("n = 0", rgb_of(g), [], {}),
             ("one mask", rgb_of(g), m3[:1], {}),
             ("overlapping masks", rgb_of(g), [np.ones((H, W), bool)] + m3 + [m3[0] & m3[1]], {})]
    white_patch = g.copy()
    white_patch[5:20, 4:30] = 255
    over = np.zeros((H, W), bool)
    over[0:25, 0:33] = True
    cases.append(("a mask over non-stroke pixels", rgb_of(white_patch), [over], {}))
    cases.append(("mask values 1, 255 and bool", rgb_of(g),
                  [m3[0].astype(np.uint8), m3[1].astype(np.uint8) * 255, m3[2]], {}))
    cases.append(("a coloured sketch", rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8), m3, {}))
    cases.append(("a single-channel sketch", g, m3, {}))
    edge = np.full((H, W), 255, np.uint8)
    edge[:, 0::2], edge[:, 1::2] = 249, 250
    edge[3, 3] = 40
    cases.append(("grey 249 and 250 side by side", rgb_of(edge), m3, {}))
    faint = strokes(rs, H, W, lo=231, hi=250)
    faint[17, 11] = 230
    cases.append(("faint, darkest pixel 230", rgb_of(faint), m3, {}))
    dark = faint.copy()
    dark[H - 1, W - 1] = 229
    cases.append(("faint but for one pixel at 229", rgb_of(dark), m3, {}))
    cases.append(("other parameters", rgb_of(g), m3,
                  dict(colors=[(255, 0, 0), (12, 200, 77), (3.5, 90.25, 254.0)], enhance_factor=2.2, min_opacity=0.35)))
    cases.append(("other parameters, faint", rgb_of(faint), m3,
                  dict(colors=[(1, 2, 3), (250, 251, 252), (128, 127, 126)], enhance_factor=0.8, min_opacity=0.6)))
    return cases
