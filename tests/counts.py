"""The integer-count checks of the texture families (oracle/counts.py), under the name the suite imports them by."""
from oracle.counts import (INT_MAX, INT_REL, INT_TOL, NGTDM_REL, TIGHT_COLUMNS, applicable, compare_counts,  # noqa: F401
                           compare_tight, recover_counts, texture_names)
