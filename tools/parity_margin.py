#!/usr/bin/env python3
"""How close each column comes to its tolerance: max over rows of |got - want| / tolerance (tests/parity.py), for every family on
the batches the GPU suite uses.  A column above 1 fails; a column that never exceeds 1e-6 has a tolerance looser than it needs.
--large: the texture families on the large-ROI batches instead (tests/test_large_rois_gpu.py, 56 k / 110 k-pixel ellipses), with the
integer-count mismatches of tests/counts.py and the worst relative difference of every NGTDM column (what sets counts.NGTDM_REL).
    python tools/parity_margin.py [--top 40] [--large]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--top", type=int, default=40)
    ap.add_argument("--large", action="store_true")
    a = ap.parse_args()
    from nyxus_amd import _abi, _lib
    from oracle import pyoracle as po
    from tests import parity, synth
    ctx = _lib.Context(0)
    if a.large:
        large(ctx, a.top)
        ctx.close()
        return
    worst = {}
    batches = [("random r25", _abi.batch_from_rois(synth.random_rois(60, seed=9, rmax=25))),
               ("random r12", _abi.batch_from_rois(synth.random_rois(60, seed=3, rmax=12))),
               ("random r40", _abi.batch_from_rois(synth.random_rois(60, seed=5, rmax=40))),
               ("irregular tile", synth.tile_batch(2, irregular=True))]
    for gd in (8, 64):
        s = _abi.default_settings(gd)
        mask = _abi.FAM_ALL & ~_abi.FAM_GABOR
        names = _lib.column_names(mask, s)
        for tag, b in batches:
            G = ctx.featurize_host(b, mask, s)
            O = po.oracle_featurize(b, mask, s)
            atol = parity.moment_atol(b, O, names)
            for j, n in enumerate(names):
                tol = parity.tolerance_of(n, O[:, j], atol=atol)
                g, w = G[:, j], O[:, j]
                same = (g == w) | (np.isnan(g) & np.isnan(w))
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.where(same, 0.0, np.abs(g - w) / tol)
                ratio = np.where(np.isnan(ratio), np.inf, ratio)
                k = int(np.argmax(ratio))
                if ratio[k] > worst.get(n, (0,))[0]:
                    med = float(np.nanmedian(np.abs(w)))
                    worst[n] = (float(ratio[k]), f"gd {gd} {tag} roi {k}: got {g[k]!r} want {w[k]!r} tol {tol[k]:.3g} median|want| {med:.3g}")
    rows = sorted(worst.items(), key=lambda kv: -kv[1][0])
    print(f"{sum(1 for _, v in rows if v[0] > 1)} columns above their tolerance; top {a.top}:")
    for n, (r, where) in rows[: a.top]:
        print(f"{r:10.3g}  {n:28s} {where}")
    ctx.close()


def large(ctx, top):
    from nyxus_amd import _abi, _lib
    from oracle import pyoracle as po
    from oracle import counts
    from tests import parity
    from tests.test_large_rois_gpu import large_rois
    from tests.test_size_classes_gpu import ellipse_roi
    rng = np.random.default_rng(71)
    extra = [ellipse_roi(150, 120, rng), ellipse_roi(210, 166, rng), ellipse_roi(210, 166, rng, lo=0, holes=0.03)]
    batches = [("large_rois", _abi.batch_from_rois(large_rois())), ("large_rois hi 200", _abi.batch_from_rois(large_rois(seed=23, hi=200))),
               ("ellipses 56k/110k", _abi.batch_from_rois(extra))]
    # the seam boxes of tests/test_texture_counts_gpu.py at the level counts where the NGTDM sums over level pairs are longest
    from tests.test_texture_counts_gpu import seam_roi, width_for
    seams = lambda hi: _abi.batch_from_rois([seam_roi(width_for(r), 3 * r + 1, r, k, rng, hi=hi) for r in (2, 63)
                                             for k in ("strip_runs", "diag135", "seam_holes", "serpentine", "noise")])
    batches += [("seam boxes", seams(4096)), ("seam boxes hi 1001", seams(1001))]
    tex = _abi.FAM_GLRLM | _abi.FAM_GLSZM | _abi.FAM_NGTDM | _abi.FAM_GLDZM | _abi.FAM_GLDM | _abi.FAM_NGLDM
    worst, ngt, n_count_bad = {}, {}, 0
    for gd, ibsi in ((8, 0), (64, 0), (-16, 0), (4094, 0), (8, 1)):
        s = _abi.default_settings(gd, bool(ibsi))
        mask = tex & ~(_abi.FAM_GLDZM | _abi.FAM_NGLDM) if gd < 0 else tex
        names = _lib.column_names(mask, s)
        for tag, b in batches:
            if (ibsi and not tag.endswith("hi 200") and not tag.endswith("hi 1001")) or (gd == 4094 and tag != "seam boxes"):
                continue
            G = ctx.featurize_host(b, mask, s)
            O = po.oracle_featurize(b, mask, s)
            where = f"gd {gd} ibsi {ibsi} {tag}"
            cb = counts.compare_counts(G, O, names)
            n_count_bad += len(cb)
            for m in cb[:5]:
                print("COUNT MISMATCH", where, m)
            for j, n in enumerate(names):
                g, w = G[:, j], O[:, j]
                same = (g == w) | (np.isnan(g) & np.isnan(w))
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.where(same, 0.0, np.abs(g - w) / parity.tolerance_of(n, w))
                    rel = np.where(same, 0.0, np.abs(g - w) / np.abs(w))
                ratio = np.where(np.isnan(ratio), np.inf, ratio)
                rel = np.where(np.isnan(rel), np.inf, rel)
                k = int(np.argmax(ratio))
                if ratio[k] >= worst.get(n, (-1,))[0]:
                    worst[n] = (float(ratio[k]), f"{where} roi {k}: got {g[k]!r} want {w[k]!r}")
                if n.startswith("NGTDM_"):
                    k = int(np.argmax(rel))
                    if rel[k] >= ngt.get(n, (-1,))[0]:
                        ngt[n] = (float(rel[k]), f"{where} roi {k}: got {g[k]!r} want {w[k]!r}")
    print(f"integer-count mismatches (tests/counts.py): {n_count_bad}")
    print("NGTDM, worst relative difference |got - want| / |want| per column:")
    for n, (r, where) in sorted(ngt.items()):
        print(f"{r:10.3g}  {n:28s} {where}")
    w = max(r for r, _ in ngt.values())
    print(f"NGTDM worst overall: {w:.3g} -> tests/counts.py NGTDM_REL = min(100 x worst, 1e-9) = {min(100 * w, 1e-9):.2g}")
    rows = sorted(worst.items(), key=lambda kv: -kv[1][0])
    print(f"{sum(1 for _, v in rows if v[0] > 1)} columns above their compare_tables tolerance; top {top} (margin = |got - want| / tolerance):")
    for n, (r, where) in rows[:top]:
        print(f"{r:10.3g}  {n:28s} {where}")


if __name__ == "__main__":
    main()
