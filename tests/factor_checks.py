"""What \"the kept factor equals the oracle's\" means, shared by the GPU test modules: ranks, first columns, total rank, column permutation,
Householder scalars and the factor itself over each problem's own rows, bit for bit."""
import numpy as np


def assert_factor_equal(s, ref, dims, nvar):
    r, fc, tr = s.getRanks()
    np.testing.assert_array_equal(r, ref["rank"])
    np.testing.assert_array_equal(fc, ref["fcol"])
    np.testing.assert_array_equal(tr, ref["totalrank"])
    np.testing.assert_array_equal(s.get_column_permutations(), ref["perm"])
    np.testing.assert_array_equal(s.get_hh_scalars(), ref["hh"])
    f = s.get_lexqr()
    dims_a = np.asarray(dims)
    m = dims_a.sum(axis=-1) if dims_a.ndim == 2 else np.full(f.shape[0], dims_a.sum())
    for b in range(f.shape[0]):
        np.testing.assert_array_equal(f[b, :, :m[b]], ref["factor"][b, :, :m[b]])
