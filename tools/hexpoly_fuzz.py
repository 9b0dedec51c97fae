"""Fuzz the hexagonality / polygonality entries (nyxhip_hexpoly_tiles, nyxhip_hexpoly_batch) against tests/hexpoly_ref.table: the random
label images of tools/neighbors_fuzz.py (discs, needles, rings with nested blobs, bridged checkerboards, combs, single pixels; dense
enough that most ROIs have three neighbors or more at the larger radii), at R in {2, 5, 12}, three images a call.  Rows whose
NUM_NEIGHBORS is at most 128 must be bit-identical to the restatement (a NaN matching a NaN), the others within 1e-5 * max(|want|, 1);
the batch entry must give the tile entry's bits.  Prints the largest difference per column.
    python tools/hexpoly_fuzz.py [seed] [rounds]"""
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from nyxus_amd import _abi, _lib
from tests import hexpoly_ref as hr, neighbors_cases as nc
from neighbors_fuzz import random_image


def main():
    ctx = _lib.Context(0)
    s = _abi.default_settings(8)
    rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
    n_bad = n_rows = n_open = n_nonfinite = 0
    worst = np.zeros(3)
    for rnd in range(int(sys.argv[2]) if len(sys.argv) > 2 else 10):
        size = int(rng.choice([48, 96, 160]))
        labs = [random_image(rng, size, int(rng.integers(10, 90))) for _ in range(3)]
        labs = [l for l in labs if l.any()]
        M = np.stack(labs)
        I = np.stack([nc.intensity(m, 900 + k) for k, m in enumerate(M)])
        b = nc.batch_of_images(labs, seed0=900)
        from tests.radial_ref import contours_of
        K = contours_of(b)
        for radius in (2, 5, 12):
            X = hr.inputs_of(b, radius, K)
            want = hr.closing_rows(X)
            tiles, labels, G = ctx.hexpoly_tiles_host(I, M, radius, s)
            B = ctx.hexpoly_host(b, radius, s)
            n_rows += len(G)
            n_open += int((want != -1).any(axis=1).sum())
            n_nonfinite += int((~np.isfinite(want)).any(axis=1).sum())
            bad = []
            if labels.tolist() != np.asarray(b.roi_label).tolist() or G.shape != want.shape:
                bad.append("rows differ")
            else:
                if G.tobytes() != B.tobytes():
                    bad.append("batch entry differs from the tile entry")
                d = np.abs(G - want)
                worst = np.maximum(worst, np.where(np.isfinite(d), d, 0.0).max(0))
                inside = X[:, 2] <= hr.TAN_TABLE_CAP
                for r in range(len(G)):
                    if inside[r]:
                        ok = hr.same_bits(G[r], want[r])
                    else:
                        fin = np.isfinite(want[r])
                        ok = (np.isnan(G[r]) == np.isnan(want[r])).all() and (np.abs(G[r][fin] - want[r][fin]) <= 1e-5 * np.maximum(np.abs(want[r][fin]), 1.0)).all()
                    if not ok:
                        bad.append(f"row {r} ({X[r].tolist()}): got {G[r].tolist()}, want {want[r].tolist()}")
            if bad:
                n_bad += len(bad)
                print("round", rnd, "R", radius, bad[:5])
    print(f"{n_rows} ROIs ({n_open} past the gates, {n_nonfinite} with NaN / inf), {n_bad} mismatches; largest difference per column "
          f"{dict(zip(hr.NAMES, worst.tolist()))}")
    sys.exit(1 if n_bad else 0)


if __name__ == "__main__":
    main()
