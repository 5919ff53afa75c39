"""Source-view selection from the pair-score matrix (host side: the matrix is N x N)."""
import numpy as np


def select_views(score, nsrc=10):
    """score [N,N] -> [N, min(nsrc, N-1)] int64: per image the other images by descending score, ties going to the lower index.
    Every image gets that many sources, zero-score ones included when nothing better is left."""
    score = np.asarray(score, dtype=np.float64)
    n = score.shape[0]
    k = max(min(int(nsrc), n - 1), 0)
    out = np.zeros((n, k), dtype=np.int64)
    for i in range(n):
        others = [j for j in range(n) if j != i]
        others.sort(key=lambda j: (-score[i, j], j))
        out[i] = others[:k]
    return out
