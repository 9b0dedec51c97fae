"""Margins of the exact GLCM check: the worst |err| / (2^-53 magnitude) per group and column over the cases of
tests/glcm_exact_cases.py, and the worst fraction of K(Ng) = Ng^2 + 2 Ng + 64 it takes, for the C oracle, the reference's own classes
(where oracle/_ref is built) and, with --hip, the HIP path (GLCM alone and INTENSITY + GLCM).  Writes the report to the given file
(default profiles/glcm_exact_margin.txt); with --hip --reports it also lists every case's launch report.

    python tools/glcm_exact_margin.py [--hip] [--reports] [--append] [out.txt]
"""
import sys

sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib                   # noqa: E402
from oracle import pyoracle as po                  # noqa: E402
from tests import glcm_exact_cases as gc           # noqa: E402
from tests import glcm_exact_ref as gx             # noqa: E402
from tests import parity                           # noqa: E402

GLCM, INT = _abi.FAM_GLCM, _abi.FAM_INTENSITY


def main(argv):
    hip, reports, append = "--hip" in argv, "--reports" in argv, "--append" in argv
    paths = [a for a in argv if not a.startswith("--")]
    out_path = paths[0] if paths else "profiles/glcm_exact_margin.txt"
    ctx = _lib.Context(0) if hip else None
    sources = ["hip GLCM", "hip INTENSITY+GLCM"] if hip else ["oracle"] + (["reference classes"] if po.have_ref() else [])
    worst = {}            # (source, group, column) -> (ratio, ratio / K, case id)
    lines, n_bad = [], 0
    for c in gc.CASES:
        b, s = gc.batch(c), c.settings()
        ex = gc.exact(c)
        tables = {}
        if hip:
            for src, mask in zip(sources, (GLCM, INT | GLCM)):
                tables[src] = (ctx.featurize_host(b, mask, s), _lib.column_names(mask, s))
                if reports:
                    lines.append("%-40s %-18s %s" % (c.id, src, [(r["class"], r["size_class"], r["rois"], r["max_side"], r["workspace"], r["cooperative"])
                                                                 for r in ctx.launch_report()]))
            want = po.oracle_featurize(b, GLCM, s)
        else:
            names = _lib.column_names(GLCM, s)
            tables["oracle"] = (po.oracle_featurize(b, GLCM, s), names)
            if po.have_ref():
                tables["reference classes"] = (po.ref_featurize(b, GLCM, s, n_threads=4), names)
        for src, (T, names) in tables.items():
            for r, e in enumerate(ex):
                ratios = {}
                bad = gx.compare_glcm_exact(T[r], e, e.Ng, names, len(e.request), ratios=ratios, tag="%s %s roi %d " % (c.id, src, r))
                n_bad += len(bad)
                lines += bad[:4]
                for col, v in ratios.items():
                    key = (src, c.group, col)
                    if v / gx.K(e.Ng) > worst.get(key, (0, -1, ""))[1]:
                        worst[key] = (v, v / gx.K(e.Ng), "%s roi %d Ng %d" % (c.id, r, e.Ng))
            if hip:
                j = [k for k, n in enumerate(names) if n.startswith("GLCM_")]
                bad = parity.compare_tables(T[:, j], want, [names[k] for k in j])
                n_bad += len(bad)
                lines += ["%s %s vs oracle: %s" % (c.id, src, m) for m in bad[:4]]
    head = ["# |err| / (2^-53 magnitude), worst over the cases of tests/glcm_exact_cases.py; 'of K' = that ratio / K(Ng) of its case (the bound is 1.0,",
            "# the CPU test holds the oracle and the reference classes to 0.25)", "# source | group | column | worst ratio | of K | where"]
    body = ["%-20s %s %-12s %10.1f %8.4f  %s" % (k[0], k[1], k[2], v[0], v[1], v[2]) for k, v in sorted(worst.items())]
    summary = []
    for src in sources:
        top = max(((v[1], k, v) for k, v in worst.items() if k[0] == src), default=None)
        if top:
            summary.append("# %s: worst %.4f of K (%s, group %s, %s)" % (src, top[0], top[1][2], top[1][1], top[2][2]))
    summary.append("# mismatches: %d" % n_bad)
    with open(out_path, "a" if append else "w") as f:
        f.write("\n".join(([] if append else head) + summary + body + lines) + "\n")
    print("\n".join(summary))
    if ctx is not None:
        ctx.close()
    return 1 if n_bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
