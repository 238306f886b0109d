"""CPU: the float64 restatement of the stain estimate (tests/stain_ref.py) against its pinned vectors
(tests/golden/make_stain_golden.py), the host half of cellsegmentation_amd.stain against the restatement, the conditions on the
fixtures that the tolerances of tests/test_stain_gpu.py rest on, the argument errors of the module, of
detect_slide(stain=...) and of measure_slide_cells(intensity=...), which are raised before the library is loaded or the model
touched, and the ABI additions with their refusals (no GPU needed)."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import stain_ref as R
from cellsegmentation_amd import _lib, inference, kernels, stain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "stain_vectors.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLD["names"]]
BIG = "synth_96x96_seed0"
SYMBOLS = ("cs_stain_moments", "cs_stain_angle_hist", "cs_stain_conc_hist", "cs_stain_apply", "cs_stain_separate")


@pytest.fixture(scope="module")
def big():
    """the reference's estimate of the 96x96 case, computed once"""
    return R.estimate(GOLD[f"{BIG}.images"])


@pytest.fixture(scope="module")
def dense():
    """the reference's estimate of the dense fixture of tests/test_stain_gpu.py: the blobs of the 96x96 case repeated 22 x 22 times
    under fresh floor and noise, 2112 x 2112 pixels"""
    return R.estimate(R.synth_hdab(96, 96, seed=0, tile=R.DENSE_TILE))


def test_od_table():
    t = stain.od_table()
    assert t.dtype == np.int32 and t.shape == (256,) and np.array_equal(t, R.od_table(240)) and np.array_equal(t, stain.od_table(240.0))
    assert t[255] == 0 and (np.diff(t) <= 0).all() and (t >= 0).all()
    # 4096 ln 240 = 22448.697: the formula of the specification rounds to 22449 (its text quotes 22448, the floor)
    assert t[0] == 22449 == int(np.rint(4096 * math.log(240.0)))
    assert t[239] == 0 and t[238] == int(np.rint(4096 * math.log(240 / 239)))
    assert stain.od_table(256)[0] == 22713 and stain.od_table(256).max() == 22713                  # 22713^2 2^31 < 2^63
    assert 22713 ** 2 * 2 ** 31 < 2 ** 63 and 8 * 22713 ** 2 < 2 ** 32
    exact = t.astype(np.float32) / np.float32(4096)
    assert np.array_equal(exact.astype(np.float64) * 4096, t)               # od_q / 4096 is exact in fp32
    for bad in (0, -1, 256.5, float("nan"), "240", True, None):
        with pytest.raises(ValueError):
            stain.od_table(bad)


def test_golden_holds_the_pinned_cases():
    assert NAMES == [BIG, "odd_37x53", "tiny_3x5", "one_pixel", "all_white", "batch_of_three"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "stain_vectors.npz")) < 1 << 20
    assert GOLD[f"{BIG}.images"].shape == (96, 96, 3) and GOLD["odd_37x53.images"].shape == (37, 53, 3)
    assert GOLD["tiny_3x5.images"].shape == (3, 5, 3) and GOLD["one_pixel.images"].shape == (1, 1, 3)
    assert (GOLD["all_white.images"] == 255).all() and GOLD["batch_of_three.images"].shape == (3, 24, 31, 3)
    assert not GOLD["all_white.ok"] and not GOLD["one_pixel.ok"] and GOLD["all_white.n_kept"] == 0 and GOLD["one_pixel.n_kept"] == 1
    assert np.array_equal(GOLD["all_white.vectors"], R.HDAB) and np.array_equal(GOLD["one_pixel.vectors"], stain.HDAB)
    assert GOLD[f"{BIG}.ok"] and GOLD["batch_of_three.ok"].all() and GOLD["batch_of_three.moments"].shape == (3, 10)
    assert len({tuple(m) for m in GOLD["batch_of_three.moments"].tolist()}) == 3                    # different content


def test_golden_regenerates():
    """integer and uint8 arrays identical; the float64 ones to 1e-12, since LAPACK's eigh and svd are not bitwise portable"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_stain_golden as G
    fresh = G.build()
    assert sorted(fresh) == sorted(GOLD.files)
    for key in GOLD.files:
        a, b = GOLD[key], fresh[key]
        assert a.dtype == b.dtype and a.shape == b.shape, key
        if a.dtype.kind == "f":
            assert np.allclose(a, b, rtol=0, atol=1e-12), key
        else:
            assert np.array_equal(a, b), key


@pytest.mark.parametrize("name", NAMES)
def test_host_half_equals_the_restatement(name):
    """stain.py's float64 arithmetic on exact numpy histograms of the reference's own angles and concentrations"""
    images = GOLD[f"{name}.images"]
    for i, image in enumerate(images if images.ndim == 4 else images[None]):
        get = lambda k: GOLD[f"{name}.{k}"][i] if images.ndim == 4 else GOLD[f"{name}.{k}"]  # noqa: E731
        m = R.moments(image)
        assert np.array_equal(m, get("moments")) and m[0] == get("n_kept")
        V, want = stain.plane_of_moments(m), R.plane(m)
        assert (V is None) == (want is None) == (not get("ok"))
        if V is None:
            continue
        assert np.allclose(V, want, rtol=0, atol=1e-12) and abs(np.linalg.norm(V, axis=0) - 1).max() < 1e-12 and (V.sum(axis=0) >= 0).all()
        e = R.estimate(image)
        assert np.allclose(e["vectors"], get("vectors"), rtol=0, atol=1e-12)
        opts = stain.StainOptions()
        hist = np.histogram(e["phi"], bins=opts.angle_bins, range=(-math.pi / 2, math.pi / 2))[0]
        S = stain.vectors_of_hist(V, hist, opts.alpha)
        for k in range(2):                                                 # half a bin of quantisation per angle
            assert R.angle_between(S[:, k], e["vectors"][:, k]) <= math.pi / opts.angle_bins / 2 + 1e-9, (name, k)
        chist = np.stack([np.histogram(np.clip(c, 0, None), bins=opts.conc_bins, range=(0, opts.conc_max))[0] for c in e["conc"]])
        mc = stain.max_conc_of_hist(chist, opts.conc_max)
        assert np.abs(mc - e["max_conc"]).max() <= opts.conc_max / opts.conc_bins / 2 + 1e-9
        A = stain.normalizer(stain.StainEstimate(e["vectors"], e["max_conc"]), stain.TARGET_HDAB)
        assert np.allclose(A, get("A"), rtol=0, atol=1e-12)
        assert stain.extreme_ranks(len(e["phi"]), 1.0) == (e["k_lo"], e["k_hi"]) == R.ranks(len(e["phi"]))


def test_vector_recovery(big):
    """On the 96x96 case the reference recovers the generator's vectors within 2 degrees (measured: 0.37 and 0.19 degrees with
    6545 of 9216 pixels kept)."""
    err = [math.degrees(R.angle_between(big["vectors"][:, k], R.HDAB[:, k])) for k in range(2)]
    print(f"kept {big['n_kept']} of 9216, recovery {err[0]:.3f} and {err[1]:.3f} degrees")
    assert big["ok"] and big["n_kept"] == 6545 and max(err) < 2.0
    assert np.array_equal(R.HDAB, stain.HDAB) and abs(np.linalg.norm(stain.HDAB, axis=0) - 1).max() < 1e-15
    assert stain.HDAB[0, 0] > stain.HDAB[0, 1]                              # haematoxylin has the larger red component


def _spans(values, k):
    return values[min(len(values) - 1, k + 10)] - values[max(0, k - 10)]


def test_angle_density(big, dense):
    """Around each chosen order statistic, the sorted phi of the ten ranks either side spans less than a quarter of an angle bin
    (pi / 4096 rad).  The histogram tests of tests/test_stain_gpu.py rest on it, so they run on the dense fixture, where it holds
    (measured: 0.0012 and 0.0088 quarter-bins with 3,493,663 pixels kept).  The 96x96 case cannot meet it -- 1.40 and 2.63
    quarter-bins: with sigma = 1.5 noise the angle of a pure-stain pixel scatters by about 0.01 rad, and 6545 kept pixels do not
    put 21 of them within 0.00077 rad at their 1st and 99th percentiles -- so the density is bought with pixels."""
    for name, e in (("96x96", big), ("dense", dense)):
        print(name, "angle spans in quarter-bins:", [_spans(e["phi"], k) / (math.pi / 4096) for k in (e["k_lo"], e["k_hi"])])
    assert dense["ok"] and dense["n_kept"] > 3_000_000
    assert max(_spans(dense["phi"], k) for k in (dense["k_lo"], dense["k_hi"])) < math.pi / 4096


def test_concentration_density(big, dense):
    """The same condition for the sorted concentrations around order statistic ceil(0.99 (n - 1)), against a quarter of
    conc_max / conc_bins = 8 / 2048 / 4, on the dense fixture (measured: 0.0011 and 0.073 quarter-bins; the 96x96 case gives 220
    and 55, its 99th percentile lying among the 65 sparse pixels of the upper tail)."""
    for name, e in (("96x96", big), ("dense", dense)):
        print(name, "concentration spans in quarter-bins:", [_spans(c, e["k_conc"]) / (8.0 / 2048 / 4) for c in e["conc"]])
    assert max(_spans(c, dense["k_conc"]) for c in dense["conc"]) < 8.0 / 2048 / 4


def test_options_and_estimates():
    o = stain.StainOptions()
    assert (o.Io, o.beta, o.alpha, o.angle_bins, o.conc_bins, o.conc_max) == (240, 0.15, 1.0, 1024, 2048, 8.0) and o.beta_q == 614
    for kw in (dict(Io=0), dict(Io=257), dict(Io="240"), dict(Io=True), dict(beta=-0.1), dict(beta=float("nan")), dict(alpha=50), dict(alpha=-1),
               dict(angle_bins=0), dict(angle_bins=8193), dict(angle_bins=10.5), dict(conc_bins=4097), dict(conc_bins=True), dict(conc_max=0),
               dict(conc_max=float("inf"))):
        with pytest.raises(ValueError):
            stain.StainOptions(**kw)
    with pytest.raises(Exception):
        o.Io = 200                                                          # frozen, as checked
    t = stain.TARGET_HDAB
    assert isinstance(t, stain.StainEstimate) and np.array_equal(t.vectors, stain.HDAB) and t.max_conc.tolist() == [1, 1] and t.ok
    for bad in (dict(vectors=np.zeros((2, 3)), max_conc=np.ones(2)), dict(vectors=stain.HDAB, max_conc=np.zeros(2)),
                dict(vectors=stain.HDAB * np.nan, max_conc=np.ones(2)), dict(vectors=stain.HDAB, max_conc=np.ones(3))):
        with pytest.raises(ValueError):
            stain.StainEstimate(**bad)
    S3 = stain.stain_matrix(stain.HDAB, residual=True)
    assert S3.shape == (3, 3) and np.allclose(S3, R.stain_matrix(R.HDAB, True)) and abs(S3[:, 2] @ S3[:, 0]) < 1e-15
    with pytest.raises(ValueError):
        stain.stain_matrix(np.stack([R.H_VEC, R.H_VEC], axis=1), residual=True)


def test_argument_errors_come_before_the_library_is_loaded(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library or the device was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(stain, "_device", no_load)
    img = np.zeros((8, 9, 3), np.uint8)
    for call in (stain.estimate, stain.normalize, stain.separate):
        for bad in (img.astype(np.float32), img.astype(np.int32), torch.zeros(8, 9, 3), [[1, 2, 3]], None):
            with pytest.raises(TypeError):
                call(bad)
        for bad in (np.zeros((8, 9), np.uint8), np.zeros((8, 9, 4), np.uint8), np.zeros((0, 9, 3), np.uint8), np.zeros((1, 2, 8, 9, 3), np.uint8)):
            with pytest.raises(ValueError):
                call(bad)
        for bad in ("x", 5, {"Io": 240}, False):
            with pytest.raises(TypeError):
                call(img, options=bad)
    for call in (stain.estimate, stain.normalize):
        for bad in (np.zeros((8, 9), np.float32), np.zeros((8, 9), np.int32), "mask"):
            with pytest.raises(TypeError):
                call(img, mask=bad)
        for bad in (np.zeros((9, 8), np.uint8), np.zeros((2, 8, 9), np.uint8), np.zeros((8, 9, 3), np.uint8)):
            with pytest.raises(ValueError):
                call(img, mask=bad)
    for bad in (stain.HDAB, "hdab", [stain.TARGET_HDAB, stain.TARGET_HDAB]):
        with pytest.raises(TypeError):
            stain.normalize(img, source=bad)
    with pytest.raises(TypeError):
        stain.normalize(img, target=stain.HDAB)
    for bad in ("u16", None, np.uint8):
        with pytest.raises(ValueError):
            stain.separate(img, dtype=bad)
    for bad in (np.zeros((2, 3)), np.full((3, 2), np.nan), np.zeros((3, 3))):
        with pytest.raises(ValueError):
            stain.separate(img, stains=bad)
    # the raw bindings refuse host tensors of the wrong type or shape before they load anything either
    x, od = torch.zeros(1, 8, 9, 3, dtype=torch.uint8), torch.zeros(256, dtype=torch.int32)
    with pytest.raises(TypeError):
        kernels.stain_moments(torch.zeros(1, 8, 9, 3), od, 614)
    with pytest.raises(ValueError):
        kernels.stain_moments(x, od[:255], 614)
    with pytest.raises(ValueError):
        kernels.stain_moments(x, od, 614, mask=torch.zeros(1, 9, 8, dtype=torch.uint8))
    with pytest.raises(ValueError):
        kernels.stain_moments(x, od, 614, out=torch.zeros(1, 9, dtype=torch.int64))
    with pytest.raises(ValueError):
        kernels.stain_angle_hist(x, od, 614, torch.zeros(1, 2, 3), 1024)
    with pytest.raises(ValueError):
        kernels.stain_conc_hist(x, od, 614, torch.zeros(1, 3, 2), 2048, 8.0)
    with pytest.raises(ValueError):
        kernels.stain_apply(x, od, torch.zeros(1, 3, 3, dtype=torch.float64), 240)
    with pytest.raises(ValueError):
        kernels.stain_separate(x, od, torch.zeros(1, 4, 3))


def test_detect_slide_checks_stain_before_the_model(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library or the device was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    img = np.zeros((80, 80, 3), np.uint8)

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the model was touched: {name}")

    for bad in (object(), "macenko", 1, False, {"Io": 240}, (stain.StainOptions(), stain.HDAB), (stain.TARGET_HDAB, stain.StainOptions()),
                (stain.StainOptions(),)):
        with pytest.raises(TypeError, match="stain"):
            inference.detect_slide(img, Untouchable(), patch_size=64, interval=48, stain=bad)
        with pytest.raises(TypeError, match="stain"):
            list(inference.detect_slides([img], Untouchable(), patch_size=64, interval=48, stain=bad))
    assert stain._check_slide_argument(True, "x") == (stain.StainOptions(), stain.TARGET_HDAB)
    mine = stain.StainEstimate(stain.HDAB[:, ::-1], [2.0, 3.0])
    assert stain._check_slide_argument((None, mine), "x") == (stain.StainOptions(), mine)
    assert stain._check_slide_argument(stain.StainOptions(alpha=2), "x")[0].alpha == 2
    # the result record: its positional fields are unchanged, the estimate is an attribute beside them
    r = inference.SlideResult(np.zeros((0, 2), np.int64), [], 0, torch.zeros(2, 2, dtype=torch.uint8))
    assert r.stain is None and r.tissue is None
    res = inference.SlideResult(np.zeros((0, 2), np.int64), [], 0, torch.zeros(4, 4, dtype=torch.uint8))
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 5), np.uint8), np.zeros((1, 4, 4), np.uint8), "dab"):
        with pytest.raises(TypeError, match="intensity"):
            inference.measure_slide_cells(res, intensity=bad)


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols()
    assert [len(_lib._SIGNATURES[n][1]) for n in SYMBOLS] == [9, 11, 12, 9, 11]
    assert _lib._SIGNATURES["cs_stain_conc_hist"][1][9] is _lib.c_float and _lib._SIGNATURES["cs_stain_apply"][1][6] is _lib.c_float
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.cs_abi_version() == 10
    src = open(os.path.join(ROOT, "cellsegmentation_amd", "csrc", "stain.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "logf" not in code and "log(" not in code, "plain C++, and no kernel calls log"
    assert "stain.hip" in open(os.path.join(ROOT, "cellsegmentation_amd", "csrc", "Makefile")).read()


def test_entry_points_refuse_bad_calls_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()                                          # host memory: nothing is launched
    base = ctypes.addressof(buf)
    base += -base % 16
    P, F = ctypes.c_void_p, ctypes.c_float

    def moments(img=base, N=1, H=4, W=4, od=base, out=base):
        return lib.cs_stain_moments(P(img), N, H, W, P(od), 614, None, P(out), None)

    def angle(img=base, N=1, H=4, W=4, od=base, V=base, bins=1024, out=base):
        return lib.cs_stain_angle_hist(P(img), N, H, W, P(od), 614, None, P(V), bins, P(out), None)

    def conc(img=base, N=1, H=4, W=4, od=base, Pm=base, bins=2048, cmax=8.0, out=base):
        return lib.cs_stain_conc_hist(P(img), N, H, W, P(od), 614, None, P(Pm), bins, F(cmax), P(out), None)

    def apply(img=base, N=1, H=4, W=4, od=base, A=base, Io=240.0, out=base + 64):
        return lib.cs_stain_apply(P(img), N, H, W, P(od), P(A), F(Io), P(out), None)

    def separate(img=base, N=1, H=4, W=4, od=base, Pm=base, K=2, u8=0, cmax=8.0, out=base):
        return lib.cs_stain_separate(P(img), N, H, W, P(od), P(Pm), K, u8, F(cmax), P(out), None)

    shapes = (dict(N=0), dict(N=65536), dict(H=0), dict(W=-1), dict(H=46341, W=46341), dict(img=None), dict(od=None), dict(out=None),
              dict(od=base + 2))
    for what, fn, cases in (
        ("stain_moments", moments, shapes + (dict(out=base + 4),)),
        ("stain_angle_hist", angle, shapes + (dict(V=None), dict(V=base + 1), dict(bins=0), dict(bins=8193), dict(out=base + 4))),
        ("stain_conc_hist", conc, shapes + (dict(Pm=None), dict(bins=0), dict(bins=4097), dict(cmax=0.0), dict(cmax=-1.0),
                                            dict(cmax=float("inf")), dict(cmax=float("nan")))),
        ("stain_apply", apply, shapes + (dict(A=None), dict(A=base + 3), dict(Io=0.0), dict(Io=257.0), dict(Io=float("nan")))),
        ("stain_separate", separate, shapes + (dict(Pm=None), dict(K=1), dict(K=4), dict(u8=2), dict(u8=1, cmax=0.0), dict(out=base + 2))),
    ):
        for kw in cases:
            assert fn(**kw) == -1, (what, kw)
            assert what.encode() in lib.cs_last_error(), (what, kw, lib.cs_last_error())
