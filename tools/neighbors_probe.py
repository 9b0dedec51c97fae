"""Cost of the neighbor entries (nyxhip_neighbors_tiles / nyxhip_neighbors_batch): ms per call, host to host (copies included), median of
`reps` after a warm-up, on
  the benchmark's tiles   `tiles` copies (default 1000) of the 1024 x 1024 tile of 196 discs bench.py featurizes, one image per tile, as
                          uint16 labels / uint8 intensities; for scale the same stack through nyxhip_featurize_tiles_v2 with ROI_RADIUS
                          alone, which pays for the same label scan, ROI assembly, clouds and contour chain but for no pair scan;
  one 2048 x 2048 image   4096 small ROIs (discs of radius 2..7 on a jittered 32-pixel lattice), through the tile entry and through the
                          batch entry.
    python tools/neighbors_probe.py [tiles] [reps]
inputs() hands the same label images to tests/golden/neighbors/make_neighbors_golden.py, which times the reference's class on them."""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from tests import synth  # noqa: E402
from tests.radial_cases import disc  # noqa: E402


def big_image(size=2048, pitch=32, seed=5):
    rng = np.random.default_rng(seed)
    lab = np.zeros((size, size), np.uint32)
    k = 0
    for gy in range(size // pitch):
        for gx in range(size // pitch):
            k += 1
            r = int(rng.integers(2, 8))
            m = disc(r)
            y = gy * pitch + int(rng.integers(0, pitch - 2 * r - 1))
            x = gx * pitch + int(rng.integers(0, pitch - 2 * r - 1))
            lab[y:y + 2 * r + 1, x:x + 2 * r + 1][m] = k
    return lab


def inputs(n_bench_tiles=8):
    return [("the benchmark's tile", [synth.disk_label_tile()] * n_bench_tiles), ("one 2048 x 2048 image of 4096 small ROIs", [big_image()])]


def timed(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return np.array(t) * 1e3


def main():
    from nyxus_amd import _abi, _lib
    from tests import neighbors_cases as nc
    n_tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = _lib.Context(0)
    s = _abi.default_settings(64)
    lab = synth.disk_label_tile().astype(np.uint16)
    M = np.ascontiguousarray(np.broadcast_to(lab, (n_tiles,) + lab.shape))
    I = np.ones(M.shape, np.uint8)
    for radius in (5, 12):
        t = timed(lambda: ctx.neighbors_tiles_host(I, M, radius, s), reps)
        n = len(ctx.neighbors_tiles_host(I, M, radius, s)[1])
        print(f"benchmark tiles: {n_tiles} tiles, {n} ROIs, R = {radius}: neighbors_tiles median {np.median(t):.2f} ms, min {t.min():.2f} ms "
              f"= {np.median(t) / n_tiles:.4f} ms per tile (host call, copies included)")
    t = timed(lambda: ctx.featurize_tiles_host(I, M, _abi.FAM_ROI_RADIUS, s), reps)
    print(f"benchmark tiles: {n_tiles} tiles, ROI_RADIUS alone through featurize_tiles (scan, assembly, clouds, contour chain; no pair scan): "
          f"median {np.median(t):.2f} ms, min {t.min():.2f} ms = {np.median(t) / n_tiles:.4f} ms per tile")
    big = big_image()
    Mb = big[None]
    Ib = np.ones(Mb.shape, np.uint8)
    b = nc.batch_of_images([big])
    for radius in (5, 12):
        t = timed(lambda: ctx.neighbors_tiles_host(Ib, Mb, radius, s), reps)
        T = ctx.neighbors_tiles_host(Ib, Mb, radius, s)[2]
        t2 = timed(lambda: ctx.neighbors_host(b, radius, s), reps)
        print(f"2048 x 2048 image: {len(T)} ROIs, R = {radius}: neighbors_tiles median {np.median(t):.3f} ms, min {t.min():.3f} ms; "
              f"neighbors_batch median {np.median(t2):.3f} ms, min {t2.min():.3f} ms; mean NUM_NEIGHBORS {T[:, 0].mean():.2f}")
    t = timed(lambda: ctx.featurize_tiles_host(Ib, Mb, _abi.FAM_ROI_RADIUS, s), reps)
    print(f"2048 x 2048 image: ROI_RADIUS alone through featurize_tiles: median {np.median(t):.3f} ms, min {t.min():.3f} ms")


if __name__ == "__main__":
    main()
