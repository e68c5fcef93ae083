"""oracle.match against an independent NumPy formulation of the two-way Match (match_cases.numpy_match:
full popcount-table distance matrix, per-row and per-column best with the delta rule, cross-check):
pins the reference that the GPU cases of test_gpu_match_paths.py lean on, at shapes on both sides
of the kernels' B-count thresholds and at every (maxDist, minDiff) class they distinguish.  CPU only."""
import numpy as np
import pytest

from match_cases import dm_bytes, match_sets, numpy_match


@pytest.mark.parametrize("na,nb", [(33, 97), (513, 3000), (300, 2560)])
def test_oracle_match_equals_numpy(oracle, na, nb):
    A, B = match_sets(na, nb, na * 7 + nb)
    for md, mdiff in ((30, 0), (30, 1), (127, 2), (128, 1), (256, 0)):
        o = oracle.match(A, B, max_distance=md, min_difference=mdiff)
        r = numpy_match(A, B, md, mdiff)
        assert len(o) > 0
        assert np.array_equal(dm_bytes(o), dm_bytes(r)), (na, nb, md, mdiff, len(o), len(r))
