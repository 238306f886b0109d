"""Writes tests/golden/stain_vectors.npz: small RGB images and what the float64 restatement tests/stain_ref.py returns for them -- the
integer moments of the kept pixels, the estimated stain vectors with ``max_conc``, ``n_kept`` and ``ok``, the image normalised to
Ruifrok's vectors with unit range, and the H-DAB separation as float64 and uint8 concentrations, with two stains and with the
residual as a third.  A batch holds one of each per image.  Inputs and recorded results only.

    python tests/golden/make_stain_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import stain_ref as R  # noqa: E402


def cases():
    """[(name, images)]: uint8 [H, W, 3], or [N, H, W, 3] for a batch"""
    rng = np.random.RandomState(11)
    other = np.stack([R.DAB_VEC, R.H_VEC[[2, 0, 1]]], axis=1)              # a batch member with stains of its own
    batch = np.stack([R.synth_hdab(24, 31, seed=3), R.synth_hdab(24, 31, seed=4, S=other),
                      rng.randint(0, 256, size=(24, 31, 3)).astype(np.uint8)])
    return [("synth_96x96_seed0", R.synth_hdab(96, 96, seed=0)),
            ("odd_37x53", R.synth_hdab(37, 53, seed=1)),
            ("tiny_3x5", R.synth_hdab(3, 5, seed=2, n_h=2, n_dab=1)),
            ("one_pixel", np.asarray([[[90, 80, 150]]], np.uint8)),
            ("all_white", np.full((20, 24, 3), 255, np.uint8)),
            ("batch_of_three", batch)]


def record_one(image):
    e = R.estimate(image)
    v = {"moments": R.moments(image), "vectors": e["vectors"], "max_conc": e["max_conc"], "n_kept": np.asarray(e["n_kept"], np.int64),
         "ok": np.asarray(e["ok"]), "A": R.normalizer(e["vectors"], e["max_conc"])}
    v["normalized"] = R.apply(image, v["A"])[0]
    for key, residual in (("sep", False), ("sep3", True)):
        v[key] = R.separate(image, R.HDAB, residual)[0]
        v[key + "_u8"] = R.separate_u8(image, R.HDAB, residual)
    return v


def record(images):
    """name -> array for one case; a batch stacks its images' records"""
    if images.ndim == 3:
        return {"images": images, **record_one(images)}
    per = [record_one(im) for im in images]
    return {"images": images, **{k: np.stack([p[k] for p in per]) for k in per[0]}}


def build():
    vec, names = {}, []
    for name, images in cases():
        names.append(name)
        for key, a in record(images).items():
            vec[f"{name}.{key}"] = a
    vec["names"] = np.asarray(names)
    return vec


def main():
    vec = build()
    g = lambda k: vec[k]  # noqa: E731
    assert g("synth_96x96_seed0.ok") and g("odd_37x53.ok") and g("batch_of_three.ok").all()
    assert not g("one_pixel.ok") and not g("all_white.ok") and g("all_white.n_kept") == 0 and g("one_pixel.n_kept") == 1
    assert np.array_equal(g("all_white.vectors"), R.HDAB) and np.array_equal(g("one_pixel.vectors"), R.HDAB)
    assert g("batch_of_three.moments").shape == (3, 10) and g("synth_96x96_seed0.sep3").shape == (96, 96, 3)
    path = os.path.join(HERE, "stain_vectors.npz")
    np.savez_compressed(path, **vec)
    print(f"{len(vec['names'])} cases written, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
