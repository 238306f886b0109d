"""Pure-numpy restatement of the per-component measurements (cellsegmentation_amd.regions.measure), the reference of
tests/test_props_gpu.py: ``regions_ref.label``, then bincount / add.at / minimum.at / maximum.at per label into the table layout
of ``RegionTable``.  Pinned to scipy.ndimage (label, sum, mean, maximum, center_of_mass, find_objects) by
tests/golden/props_vectors.npz (tests/test_props_host.py); scipy is not imported here.

Row k of image n is scipy label k + 1; rows at or above min(count, capacity) are all zero.
"""
import numpy as np

import regions_ref as R


def _one(m, v, connectivity, cap):
    """tables of one [H, W] mask with a fixed capacity, from its label image"""
    lab, count = R.label(m, connectivity)
    H, W = m.shape
    rr, cc = np.nonzero(lab)
    k = lab[rr, cc].astype(np.int64) - 1
    keep = k < cap
    rr, cc, k = rr[keep], cc[keep], k[keep]
    area = np.bincount(k, minlength=cap).astype(np.int32)
    sums = np.zeros((cap, 2), np.int64)
    np.add.at(sums[:, 0], k, rr)
    np.add.at(sums[:, 1], k, cc)
    big = np.iinfo(np.int32).max
    bbox = np.zeros((cap, 4), np.int32)
    bbox[:, :2] = big
    np.minimum.at(bbox[:, 0], k, rr)
    np.minimum.at(bbox[:, 1], k, cc)
    np.maximum.at(bbox[:, 2], k, rr + 1)
    np.maximum.at(bbox[:, 3], k, cc + 1)
    bbox[area == 0] = 0
    out = {"count": np.int32(count), "area": area, "bbox": bbox, "sum_rc": sums}
    if v is not None:
        isum = np.zeros(cap, np.int64)
        imax = np.zeros(cap, np.int32)
        np.add.at(isum, k, v[rr, cc].astype(np.int64))
        np.maximum.at(imax, k, v[rr, cc].astype(np.int32))
        out["intensity_sum"], out["intensity_max"] = isum, imax
    return out


def count(m, connectivity=1):
    m = np.asarray(m)
    return np.asarray([R.label(x, connectivity)[1] for x in (m[None] if m.ndim == 2 else m)], np.int32)


def measure(m, intensity=None, connectivity=1, max_regions=None):
    """m bool [H, W] or [N, H, W]; intensity uint8 of the same shape or None -> dict: counts int32 [N], capacity, area int32
    [N, cap], bbox int32 [N, cap, 4] (r0, c0, r1, c1), sum_rc int64 [N, cap, 2] and, with intensity, intensity_sum int64
    [N, cap] and intensity_max int32 [N, cap].  max_regions None: capacity = the largest count (1 when there is no component)."""
    m = np.asarray(m)
    if m.ndim == 2:
        m = m[None]
        intensity = None if intensity is None else np.asarray(intensity)[None]
    cap = max(1, int(count(m, connectivity).max())) if max_regions is None else int(max_regions)
    per = [_one(x, None if intensity is None else np.asarray(intensity[i]), connectivity, cap) for i, x in enumerate(m)]
    out = {"counts": np.asarray([p["count"] for p in per], np.int32), "capacity": cap}
    for key in per[0]:
        if key != "count":
            out[key] = np.stack([p[key] for p in per])
    return out


def centroid(t):
    """float64 [N, cap, 2] = sum_rc / area, NaN in unused rows"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return t["sum_rc"].astype(np.float64) / t["area"].astype(np.float64)[..., None]


def mean_intensity(t):
    with np.errstate(invalid="ignore", divide="ignore"):
        return t["intensity_sum"].astype(np.float64) / t["area"].astype(np.float64)


def per_image(t):
    """RegionTable.per_image of the dict above: a list of dicts trimmed to min(count, capacity)"""
    out = []
    for n, c in enumerate(t["counts"]):
        k = min(int(c), t["capacity"])
        d = {"area": t["area"][n, :k], "bbox": t["bbox"][n, :k], "centroid": centroid(t)[n, :k]}
        if "intensity_sum" in t:
            d["intensity_sum"], d["intensity_max"] = t["intensity_sum"][n, :k], t["intensity_max"][n, :k]
            d["intensity_mean"] = mean_intensity(t)[n, :k]
        out.append(d)
    return out
