"""Margins of the exact 3-D GLCM check (tests/vol_exact_ref.py): per column the worst |err| / (2^-53 magnitude) as a fraction of
K(Ng) = Ng^2 + 2 Ng + 64,

  * of the reference's own 3-D classes, over the 15 recorded cases of tests/golden/vol/vol_reference.npz (what the scale asserted in
    tests/test_vol_exact_cpu.py is measured on), and of the NumPy restatement tests/vol_ref.py on the same cases;
  * with --hip, of the HIP path (VFAM_GLCM and VFAM_ALL) over the recorded cases and the cases of tests/vol_edge_cases.py.  That part can
    only be measured on the GPU; without --hip the HIP lines already in the file are kept.

    python tools/vol_glcm_exact_margin.py [--hip] [out.txt]          (default profiles/vol_glcm_exact_margin.txt)
"""
import os
import sys

import numpy as np

sys.path.insert(0, ".")
from nyxus_amd import _abi                             # noqa: E402
from tests import vol_cases, vol_edge_cases as ve      # noqa: E402
from tests import vol_exact_ref as vx                  # noqa: E402
from tests import vol_ref                              # noqa: E402

SCALE = 0.25                                           # tests/test_vol_exact_cpu.py
N_INT = vol_cases.N_INT


def fold(worst, src, T, rows, names, where, lines):
    n_bad = 0
    for r, e in enumerate(rows):
        ratios = {}
        bad = vx.compare_vol_exact(T[r], e, e.Ng, names, ratios=ratios, tag="%s %s roi %d " % (src, where, r))
        n_bad += len(bad)
        lines += bad[:4]
        for col, v in ratios.items():
            if v / vx.K(e.Ng) > worst.get((src, col), (0, -1, ""))[1]:
                worst[(src, col)] = (v, v / vx.K(e.Ng), "%s roi %d Ng %d" % (where, r, e.Ng))
    return n_bad


def main(argv):
    hip = "--hip" in argv
    paths = [a for a in argv if not a.startswith("--")]
    out_path = paths[0] if paths else "profiles/vol_glcm_exact_margin.txt"
    names = vx.glcm_names()
    gold = np.load(os.path.join("tests", "golden", "vol", "vol_reference.npz"))
    worst, lines, n_bad = {}, [], 0
    per_case = []
    ctx = None
    if hip:
        from nyxus_amd import _lib
        ctx = _lib.Context(0)
    for bname, mode in vol_cases.CASES:
        b, s = vol_cases.batch(bname), vol_cases.settings(mode)
        rows = vx.exact_rows(b, s)
        where = vol_cases.case_name(bname, mode)
        n_bad += fold(worst, "reference classes", gold[where][:, N_INT:], rows, names, where, lines)
        case = {}
        n_bad += fold(case, "reference classes", gold[where][:, N_INT:], rows, names, where, [])
        top = max(case.items(), key=lambda kv: kv[1][1], default=(("", "-"), (0, 0, "")))
        per_case.append("# reference classes %-24s worst %.4f of K (%s)" % (where, top[1][1], top[0][1]))
        n_bad += fold(worst, "vol_ref", vol_ref.glcm_rows(b, s), rows, names, where, lines)
        if hip:
            n_bad += fold(worst, "hip GLCM", ctx.volumes_host(b, _abi.VFAM_GLCM, s), rows, names, where, lines)
            n_bad += fold(worst, "hip ALL", ctx.volumes_host(b, _abi.VFAM_ALL, s)[:, N_INT:], rows, names, where, lines)
    if hip:
        for c in ve.GLCM_CASES:
            b, s = ve.batch(c.bname), ve.settings(c.mode)
            n_bad += fold(worst, "hip GLCM", ctx.volumes_host(b, _abi.VFAM_GLCM, s), ve.exact(c), names, c.id, lines)
            n_bad += fold(worst, "hip ALL", ctx.volumes_host(b, _abi.VFAM_ALL, s)[:, N_INT:], ve.exact(c), names, c.id, lines)
        ctx.close()
    kept = []
    if not hip and os.path.exists(out_path):
        kept = [l.rstrip("\n") for l in open(out_path) if l.startswith("hip ") or l.startswith("# hip ")]
    sources = ["reference classes", "vol_ref"] + (["hip GLCM", "hip ALL"] if hip else [])
    ref_top = max(v[1] for k, v in worst.items() if k[0] == "reference classes")
    head = ["# |err| / (2^-53 magnitude) of the 24 rational 3-D GLCM columns and their _AVE twins against tests/vol_exact_ref.py, worst per column;",
            "# 'of K' = that ratio / K(Ng) of its ROI, K(Ng) = Ng^2 + 2 Ng + 64 (the a-priori bound is 1.0 of K).",
            "# reference classes, vol_ref: over the 15 recorded cases of tests/golden/vol; hip: those and the cases of tests/vol_edge_cases.py.",
            "# asserted scale for the reference's classes and vol_ref (tests/test_vol_exact_cpu.py): %g of K; measured worst of the reference's classes"
            " %.4f of K: headroom %.1f x" % (SCALE, ref_top, SCALE / ref_top),
            "# the HIP path is held to 1.0 of K, which is derived; its measured ratios are recorded, not asserted"]
    summary = []
    for src in sources:
        top = max(((v[1], k, v) for k, v in worst.items() if k[0] == src), default=None)
        if top:
            summary.append("# %s: worst %.4f of K (%s, %s)" % (src, top[0], top[1][1], top[2][2]))
    summary.append("# mismatches: %d" % n_bad)
    body = ["# source | column | worst ratio | of K | where"]
    body += ["%-18s %-16s %10.1f %8.4f  %s" % (k[0], k[1], v[0], v[1], v[2]) for k, v in sorted(worst.items())]
    with open(out_path, "w") as f:
        f.write("\n".join(head + per_case + summary + body + kept + lines) + "\n")
    print("\n".join(summary))
    return 1 if n_bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
