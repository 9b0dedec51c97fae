"""Fuzz of nyxhip_wsgroup_slides against the numpy restatement tests/wsgroup_ref.py: random shapes of 1 .. 300 pixels a side with the band
seams (WS_BAND_PIXELS / w rows, one less, one more) and sides 1 and 2 over-sampled; uint8 / uint16 / uint32; zeros, flat patches and
32-bit values.  Prints the largest relative difference of the contour and radial blocks (contour and FRAC_AT_D / MEAN_FRAC must be 0) and,
for the two moment blocks, the largest difference as a share of the tolerance tests/parity.py grants the column on that slide (central
moments that cancel have a floor there: a relative figure means nothing for them).
    python tools/wsgroup_fuzz.py [n_slides] [seed]"""
import sys
import numpy as np
sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib
from tests import parity, wsgroup_ref as wr
from tests.wholeslide_cases import slide_batch

n_slides = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
ctx = _lib.Context(0)
s = _abi.default_settings(64)
B = _abi.WS_BAND_PIXELS
worst = {"contour": 0.0, "smoms": 0.0, "imoms": 0.0, "frac/mean": 0.0, "cv": 0.0}
where = {}
for k in range(n_slides):
    pick = rng.integers(0, 4)
    if pick == 0:                                               # a band seam
        w = int(rng.integers(55, 301))
        h = max(1, min(300, B // w + int(rng.integers(-1, 2)) + (B // w) * int(rng.integers(0, 2))))
    elif pick == 1:                                             # a side of 1 or 2
        w, h = int(rng.integers(1, 3)), int(rng.integers(1, 301))
        if rng.integers(0, 2):
            w, h = h, w
    else:
        w, h = int(rng.integers(1, 301)), int(rng.integers(1, 301))
    dt = [np.uint8, np.uint16, np.uint32][int(rng.integers(0, 3))]
    top = {np.uint8: 256, np.uint16: 65536, np.uint32: 1 << 32}[dt]
    img = rng.integers(0, top, (h, w), dtype=np.uint64)
    kind = int(rng.integers(0, 4))
    if kind == 1:
        img *= rng.random((h, w)) > 0.4                         # zeros
    elif kind == 2:
        img[: h // 2 + 1, : w // 2 + 1] = int(rng.integers(0, top))   # a flat patch
    img = np.ascontiguousarray(img.astype(dt))
    got = ctx.wsgroup_slides_host(img[None], _abi.WS_ALL, s)[0]
    want = wr.row(img)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (w, h, dt)
    with np.errstate(all="ignore"):
        rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    rel = np.where(np.isfinite(rel) & (got != want), rel, 0.0)
    names = _lib.wsgroup_column_names(_abi.WS_SMOMS | _abi.WS_IMOMS)
    atol = parity.moment_atol(slide_batch([img]), want[None, 7:187], names)
    for j, nm in enumerate(names):                              # the moment blocks: |difference| / tolerance
        tol = float(parity.tolerance_of(nm, want[None, 7 + j], atol=atol)[0])
        d = abs(got[7 + j] - want[7 + j])
        rel[7 + j] = 0.0 if not np.isfinite(d) or d == 0 else (d / tol if tol > 0 else np.inf)
    for name, sl in (("contour", slice(0, 7)), ("smoms", slice(7, 97)), ("imoms", slice(97, 187)), ("frac/mean", slice(187, 203)), ("cv", slice(203, 211))):
        m = float(rel[sl].max())
        if m > worst[name]:
            worst[name], where[name] = m, (w, h, np.dtype(dt).name, int(np.argmax(rel[sl])))
for name, v in worst.items():
    unit = "largest difference / tolerance of tests/parity.py" if name in ("smoms", "imoms") else "largest relative difference"
    print(f"{name}: {unit} {v:.3e} {where.get(name, '')}")
assert worst["contour"] == 0 and worst["frac/mean"] == 0 and worst["smoms"] <= 1 and worst["imoms"] <= 1
ctx.close()
