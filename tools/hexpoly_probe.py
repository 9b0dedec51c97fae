"""Cost of the hexagonality / polygonality entries (nyxhip_hexpoly_tiles / nyxhip_hexpoly_batch) beside the three older calls that produce
the same six inputs: ms per call, host to host (copies included), `runs` alternating runs (default 5) in one process after a warm-up, on
  the benchmark's tiles   `tiles` copies (default 1000) of the 1024 x 1024 tile of 196 discs bench.py featurizes, one image per tile, as
                          uint16 labels / uint8 intensities, through the tile entries;
  one 2048 x 2048 image   4096 small ROIs (tools/neighbors_probe.big_image), through the batch entries.
A run is: the new entry, then neighbors_*, morph_* with CONTOUR | HULL and the family call with NYXHIP_FAM_FERET.  The new entry runs one
contour chain (and one label scan / ROI assembly on the tile path) where the three separate calls run two (three); it is reported
beside their sum with the range of the runs.
    python tools/hexpoly_probe.py [tiles] [runs]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from tests import synth  # noqa: E402


def ms(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def report(tag, calls, runs):
    """calls: [(name, f)], the new entry first.  Alternating: every run times every call once, in order."""
    for _, f in calls:
        f()
    T = np.array([[ms(f) for _, f in calls] for _ in range(runs)])
    parts = "; ".join(f"{name} {np.median(T[:, k]):.2f} ({T[:, k].min():.2f} .. {T[:, k].max():.2f})" for k, (name, _) in enumerate(calls))
    tot = T[:, 1:].sum(axis=1)
    print(f"{tag}: {parts}; sum of the three separate calls {np.median(tot):.2f} ({tot.min():.2f} .. {tot.max():.2f}) ms; "
          f"new entry / sum {np.median(T[:, 0]) / np.median(tot):.3f}")


def main():
    from nyxus_amd import _abi, _lib
    from tests import neighbors_cases as nc
    from neighbors_probe import big_image
    n_tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = _lib.Context(0)
    s = _abi.default_settings(64)
    R = 16                                   # (the benchmark tile's discs stand 13 pixels apart: at R <= 12 none has a neighbor and every row is gated)
    mm = _abi.MORPH_CONTOUR | _abi.MORPH_HULL
    lab = synth.disk_label_tile().astype(np.uint16)
    M = np.ascontiguousarray(np.broadcast_to(lab, (n_tiles,) + lab.shape))
    I = np.ones(M.shape, np.uint8)
    T = ctx.hexpoly_tiles_host(I, M, R, s)[2]
    report(f"benchmark tiles: {n_tiles} tiles, {len(T)} ROIs, R = {R}, {int((T[:, 0] != -1).sum())} past the gates (ms per call, median and range)",
           [("hexpoly_tiles", lambda: ctx.hexpoly_tiles_host(I, M, R, s)), ("neighbors_tiles", lambda: ctx.neighbors_tiles_host(I, M, R, s)),
            ("morph_tiles CONTOUR|HULL", lambda: ctx.morph_tiles_host(I, M, mm, s)), ("featurize_tiles FERET", lambda: ctx.featurize_tiles_host(I, M, _abi.FAM_FERET, s))], runs)
    big = big_image()
    b = nc.batch_of_images([big])
    for radius in (12, 30):
        T = ctx.hexpoly_host(b, radius, s)
        report(f"2048 x 2048 image: {len(T)} ROIs, R = {radius}, {int((T[:, 0] != -1).sum())} past the gates (ms per call, median and range)",
               [("hexpoly_batch", lambda: ctx.hexpoly_host(b, radius, s)), ("neighbors_batch", lambda: ctx.neighbors_host(b, radius, s)),
                ("morph_batch CONTOUR|HULL", lambda: ctx.morph_host(b, mm, s)), ("featurize_batch FERET", lambda: ctx.featurize_host(b, _abi.FAM_FERET, s))], runs)


if __name__ == "__main__":
    main()
