"""Golden vectors for tiles.sample_patches, produced by the REFERENCE's own ``MaskTestset.sample_patches``
(dataset/dataset.py:577-612).  dataset/dataset.py cannot be imported (h5py / skimage / openslide are not installed), so the method's
source text is cut out of the file with ``ast`` and executed as a plain function on a stand-in ``self`` holding ``mode`` and
``patch_size`` -- the reference's statements run unmodified, only numpy is needed (as tests/golden/make_stage_golden.py does).

    python tests/golden/make_slide_golden.py <path of the reference checkout>

Writes tests/golden/slide_vectors.npz: per case the mode, (size, patch_size, interval) and the corner array -- data only.
cellsegmentation_amd.tiles.sample_patches is asserted equal to the reference on every case before anything is written."""
import ast
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cellsegmentation_amd import tiles  # noqa: E402


def _function_source(path, name):
    src = open(path).read()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            lines = ast.get_source_segment(src, node).split("\n")
            pad = node.col_offset                                        # get_source_segment keeps later lines' indentation
            return "\n".join([lines[0]] + [l[pad:] if l[:pad].strip() == "" else l for l in lines[1:]])
    raise KeyError(name)


def _exec_function(path, name, glob):
    ns = dict(glob)
    exec(compile(_function_source(path, name), f"{path}:{name}", "exec"), ns)
    return ns[name]


def cases():
    """(mode, size, patch_size, interval): both modes, square and non-square patches, exact fits, one pixel more than a fit, an
    interval larger than the patch, a patch as large as the image."""
    out = []
    for mode in ("WSI", "ROI"):
        out += [(mode, (4096, 4096), (299, 299), (283, 283)),
                (mode, (299, 299), (299, 299), (283, 283)),              # the patch is the image
                (mode, (582, 865), (299, 299), (283, 283)),              # exact fits: 299 + 283 k
                (mode, (583, 866), (299, 299), (283, 283)),              # one pixel more than a fit
                (mode, (581, 864), (299, 299), (283, 283)),              # one pixel less
                (mode, (300, 1000), (299, 299), (283, 283)),
                (mode, (1000, 300), (299, 299), (283, 283)),
                (mode, (150, 170), (64, 64), (48, 48)),
                (mode, (210, 260), (64, 64), (48, 48)),
                (mode, (101, 131), (37, 53), (21, 37)),                  # non-square patch and interval
                (mode, (131, 101), (53, 37), (37, 21)),
                (mode, (500, 400), (64, 32), (100, 50)),                 # interval larger than the patch (gaps)
                (mode, (164, 132), (64, 32), (100, 50)),                 # ... at an exact fit
                (mode, (165, 133), (64, 32), (100, 50)),                 # ... and one pixel more
                (mode, (64, 200), (64, 16), (1, 7)),                     # one row of origins; interval 1 on the other axis is moot
                (mode, (70, 40), (64, 16), (1, 7)),
                (mode, (1024, 768, 3), (299, 299), (283, 283)),          # img.shape of an RGB ROI: the third entry is not read
                (mode, (97, 89), (16, 16), (16, 16)),                    # interval = patch: no overlap
                (mode, (96, 80), (16, 16), (16, 16)),
                (mode, (1, 5), (1, 1), (1, 2))]
    return out


def main():
    ref = sys.argv[1]
    sample = _exec_function(os.path.join(ref, "dataset/dataset.py"), "sample_patches", {"np": np})
    out, meta = {}, []
    for i, (mode, size, patch, interval) in enumerate(cases()):
        me = types.SimpleNamespace(mode=mode, patch_size=np.asarray(patch))
        want = np.asarray(sample(me, size, np.asarray(interval)), dtype=np.int64).reshape(-1, 2)
        got = np.asarray(tiles.sample_patches(size, patch, interval), dtype=np.int64).reshape(-1, 2)
        assert np.array_equal(got, want), (mode, size, patch, interval)
        out[f"case{i}/corners"] = want
        meta.append([mode == "WSI", size[0], size[1], patch[0], patch[1], interval[0], interval[1]])
    out["meta"] = np.asarray(meta, dtype=np.int64)                        # [is_wsi, size0, size1, patch0, patch1, interval0, interval1]
    # the default interval is patch_size - 16 (dataset/dataset.py:540,548)
    assert tiles.sample_patches((4096, 4096)) == tiles.sample_patches((4096, 4096), (299, 299), (283, 283))
    for mode in ("WSI", "ROI"):                                           # a patch larger than the image: the reference dies on an empty list
        for size in ((298, 400), (400, 298)):
            try:
                sample(types.SimpleNamespace(mode=mode, patch_size=np.asarray((299, 299))), size, np.asarray((283, 283)))
            except IndexError:
                continue
            raise AssertionError("the reference was expected to raise IndexError")
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "slide_vectors.npz"), **out)
    print(f"{len(meta)} cases, {sum(len(v) for k, v in out.items() if k != 'meta')} corners")


if __name__ == "__main__":
    main()
