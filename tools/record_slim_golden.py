#!/usr/bin/env python3
"""Records tests/golden/slim_ref.npz: the reference's SLIM weights on the 60 x 37 matrix of tests/slim_restate.py.

    python tools/record_slim_golden.py /path/to/reference [--out tests/golden/slim_ref.npz]

The reference's own per-column worker (`SLIM.work` of its algorithms/linear_algs.py, imported from the path given) is
called one column at a time, so that sklearn's ConvergenceWarning can be told per column; its coordinate draws come
from numpy's global generator, seeded here.  A column that sklearn did not bring below its tolerance before max_iter
makes the recording fail: the test compares objectives within tol G_jj, which holds only between converged solves.
One case is told apart: an item nobody holds has y = 0, so sklearn's tolerance tol * y.y is 0 and its strict test
`gap < tol` reads 0 < 0 for ever; it warns after max_iter sweeps that changed nothing.  Such a column counts as
converged when the worker returned no weight for it: w = 0 has gap 0 and P_j(0) = 0 is the minimum.
Needs scikit-learn and scipy; the test suite needs neither to read the file.
"""
import argparse
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))

ALPHA, L1_RATIO, MAX_ITER, SEED = 0.01, 0.3, 200, 0


def main(argv=None) -> int:
    cli = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    cli.add_argument('reference', help='root directory of the reference project')
    cli.add_argument('--out', default=os.path.join(HERE, '..', 'tests', 'golden', 'slim_ref.npz'))
    opts = cli.parse_args(argv)
    import scipy.sparse as sp
    from sklearn.exceptions import ConvergenceWarning
    import slim_restate as sr
    sys.path.insert(0, os.path.abspath(opts.reference))
    from algorithms.linear_algs import SLIM

    X = sr.golden_matrix()
    n_users, n_items = X.shape
    A = sp.csc_matrix(X)
    W = np.zeros((n_items, n_items))
    converged = np.zeros(n_items, dtype=bool)
    np.random.seed(SEED)
    for j in range(n_items):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            rows, cols, data = SLIM.work([j, j + 1, A, ALPHA, L1_RATIO, MAX_ITER])
        warned = any(issubclass(c.category, ConvergenceWarning) for c in caught)
        converged[j] = not warned or (not X[:, j].any() and len(data) == 0)
        assert all(c == j for c in cols)
        W[np.asarray(rows, dtype=np.int64), j] = data
    assert np.array_equal(A.toarray(), X), 'the worker did not restore the matrix'
    if not converged.all():
        print(f'columns {np.nonzero(~converged)[0].tolist()} did not converge within {MAX_ITER} sweeps: nothing written')
        return 1
    np.savez(opts.out, X=X.astype(np.int8), alpha=np.float64(ALPHA), l1_ratio=np.float64(L1_RATIO),
             max_iter=np.int64(MAX_ITER), tol=np.float64(sr.TOL), seed=np.int64(SEED), W=W, converged=converged)
    print(f'{opts.out}: W {W.shape}, {int((W > 0).sum())} weights above 0, all {n_items} columns converged')
    return 0


if __name__ == '__main__':
    sys.exit(main())
