"""Fuzz the neighbor entries (nyxhip_neighbors_tiles, nyxhip_neighbors_batch) against tests/neighbors_ref.py: random label images of
discs, needles, rings with nested blobs, bridged checkerboards, combs and single pixels, dense enough that boxes overlap and shapes
touch, at R in {1, 2, 5, 12}, three images a call.  NUM_NEIGHBORS, PERCENT_TOUCHING, the two distances and the mode must be
bit-identical to the restatement, the angle columns within 1e-5 (the device's atan2 is not libm's); the batch entry must give the tile
entry's bits.
    python tools/neighbors_fuzz.py [seed] [rounds]"""
import sys

import numpy as np

sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib
from tests import neighbors_cases as nc, neighbors_ref as nr
from tests.circle_cases import checkerboard
from tests.radial_cases import comb, disc


def random_shape(rng):
    kind = int(rng.integers(0, 8))
    if kind == 0:
        return disc(int(rng.integers(1, 10)))
    if kind == 1:                                                            # a needle along a slope
        h, w = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        yy, xx = np.mgrid[0:h, 0:w]
        return yy == (xx * max(h - 1, 0)) // max(w - 1, 1)
    if kind == 2:                                                            # a ring: blobs may land in its hole
        r = int(rng.integers(6, 20))
        q = int(rng.integers(2, r - 2))
        return disc(r) & ~np.pad(disc(q), r - q)
    if kind == 3:
        return checkerboard()[:int(rng.integers(3, 12)), :int(rng.integers(3, 14))]
    if kind == 4:
        return np.ones((1, 1), bool) if rng.random() < 0.5 else np.ones((1, 2), bool)
    if kind == 5:
        return comb(int(rng.integers(1, 6)), int(rng.integers(2, 12)), spine=2)
    if kind == 6:
        return np.ones((int(rng.integers(1, 12)), int(rng.integers(1, 12))), bool)
    return rng.random((int(rng.integers(2, 14)), int(rng.integers(2, 14)))) < 0.7


def random_image(rng, size, n_shapes):
    lab = np.zeros((size, size), np.uint32)
    label = 0
    for _ in range(n_shapes):
        m = random_shape(rng)
        if not m.any() or m.shape[0] > size or m.shape[1] > size:
            continue
        y, x = int(rng.integers(0, size - m.shape[0] + 1)), int(rng.integers(0, size - m.shape[1] + 1))
        win = lab[y:y + m.shape[0], x:x + m.shape[1]]
        m = m & (win == 0)                                                   # what is free: shapes end up edge to edge
        if not m.any():
            continue
        label += int(rng.integers(1, 4))                                     # non-contiguous labels
        win[m] = label
    return lab


def main():
    ctx = _lib.Context(0)
    s = _abi.default_settings(8)
    rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
    exact = [i for i, n in enumerate(nr.NAMES) if n in nr.EXACT]
    n_bad = n_rows = n_neigh = n_touch = 0
    for rnd in range(int(sys.argv[2]) if len(sys.argv) > 2 else 10):
        size = int(rng.choice([48, 96, 160]))
        labs = [random_image(rng, size, int(rng.integers(10, 90))) for _ in range(3)]
        labs = [l for l in labs if l.any()]
        M = np.stack(labs)
        I = np.stack([nc.intensity(m, 900 + k) for k, m in enumerate(M)])
        b = nc.batch_of_images(labs, seed0=900)
        for radius in (1, 2, 5, 12):
            want = nr.table(b, radius)[:, :9]
            tiles, labels, G = ctx.neighbors_tiles_host(I, M, radius, s)
            B = ctx.neighbors_host(b, radius, s)
            n_rows += len(G)
            n_neigh += int(want[:, 0].sum())
            n_touch += int((want[:, 1] > 0).sum())
            bad = []
            if labels.tolist() != np.asarray(b.roi_label).tolist() or G.shape != want.shape:
                bad.append("rows differ")
            else:
                if G.tobytes() != B.tobytes():
                    bad.append("batch entry differs from the tile entry")
                bad += [f"row {r} {nr.NAMES[exact[c]]}: got {G[r, exact[c]]!r}, want {want[r, exact[c]]!r}" for r, c in np.argwhere(G[:, exact] != want[:, exact])[:10]]
                bad += [f"row {r} {nr.NAMES[c]}: got {G[r, c]!r}, want {want[r, c]!r}" for r, c in np.argwhere(~(np.abs(G - want) <= 1e-5 * np.abs(want)))[:10]]
            if bad:
                n_bad += len(bad)
                print("round", rnd, "R", radius, bad[:5])
    print(f"{n_rows} ROIs ({n_neigh} neighbor relations, {n_touch} touching ROIs), {n_bad} mismatches")
    sys.exit(1 if n_bad else 0)


if __name__ == "__main__":
    main()
