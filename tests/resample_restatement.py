"""NumPy restatement of the cloud resampling as include/glim_amd.h ("Resampling a resident cloud") states it: which points a random sample
keeps, the selection of the m smallest (key, index) pairs, and the transform of points, covariances and normals in FP64 with the stated
operation order.  tests/test_resample*.py check the library against this; nothing here touches the library."""
import numpy as np

from ransac_restatement import sample_hash

FULL_RATE = 0.99


def keys(n, seed):
    """the 32-bit key of every point: the upper half of the generator's word"""
    return np.array([sample_hash(seed, i) >> 32 for i in range(n)], dtype=np.uint32)


def count(n, rate):
    """points a rate keeps of n: (int64)((double)n * rate), the whole cloud from 0.99 on"""
    if rate >= FULL_RATE:
        return int(n)
    return int(float(n) * float(rate))


def select_smallest(keys32, m):
    """flags of the m lexicographically smallest (key, index)"""
    k = np.asarray(keys32, dtype=np.uint32)
    keep = np.zeros(len(k), dtype=np.int32)
    order = np.lexsort((np.arange(len(k)), k))  # the last key is the primary one
    keep[order[:m]] = 1
    return keep


def random_sample_indices(n, rate, seed):
    """ascending indices of the points random_sampling keeps"""
    m = count(n, rate)
    if m >= n:
        return np.arange(n, dtype=np.int64)
    k = keys(n, seed)
    order = np.lexsort((np.arange(n), k))
    return np.sort(order[:m]).astype(np.int64)


def transform(points4, covs6, normals3, T):
    """points4: N x 4 (x y z w), covs6: N x 6 (c00 c01 c02 c11 c12 c22) or None, normals3: N x 3 or None, all float64; T: 3 x 4 or 4 x 4.
    Every product and sum is one rounded FP64 operation, in the stated order."""
    T = np.asarray(T, dtype=np.float64)[:3, :4]
    with np.errstate(all="ignore"):
        p = np.asarray(points4, dtype=np.float64)
        q = np.empty_like(p)
        for r in range(3):
            q[:, r] = ((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] * p[:, 3]
        q[:, 3] = p[:, 3]
        d = None
        if covs6 is not None:
            c = np.asarray(covs6, dtype=np.float64)
            C = [[c[:, 0], c[:, 1], c[:, 2]], [c[:, 1], c[:, 3], c[:, 4]], [c[:, 2], c[:, 4], c[:, 5]]]
            LC = [[(T[r, 0] * C[0][k] + T[r, 1] * C[1][k]) + T[r, 2] * C[2][k] for k in range(3)] for r in range(3)]
            d = np.stack([(LC[r][0] * T[k, 0] + LC[r][1] * T[k, 1]) + LC[r][2] * T[k, 2] for r in range(3) for k in range(r, 3)], axis=1)
        m = None
        if normals3 is not None:
            v = np.asarray(normals3, dtype=np.float64)
            m = np.stack([(T[r, 0] * v[:, 0] + T[r, 1] * v[:, 1]) + T[r, 2] * v[:, 2] for r in range(3)], axis=1)
    return q, d, m


def cov6(c33):
    """N x 3 x 3 -> N x 6, the upper triangle by rows"""
    c = np.asarray(c33)
    return np.stack([c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]], axis=1)


def cov33(c6):
    """N x 6 -> N x 3 x 3, symmetric"""
    c = np.asarray(c6)
    return np.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], axis=1).reshape(-1, 3, 3)
