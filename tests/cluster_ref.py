"""The rule of jtk_batch_minhash_cluster in plain Python, written from its text (include/jtokkit_amd.h) alone: a dict per band
for the buckets, a list for the union-find.  Nothing here is shared with the kernels."""
import numpy as np


def cluster(sig, band_keys, min_agree, n_shingles=None):
    """(labels int64 [n], rep int64 [n, B]) for sig uint32 [n, K], band_keys uint64 [n, B], n_shingles int32 [n] or None."""
    n, bands = band_keys.shape
    live = [n_shingles is None or n_shingles[d] > 0 for d in range(n)]
    rep = np.full((n, bands), -1, dtype=np.int64)
    for j in range(bands):
        smallest = {}                                    # key -> the smallest live index that has it in band j
        for d in range(n):
            if live[d]:
                rep[d, j] = smallest.setdefault(int(band_keys[d, j]), d)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for d in range(n):
        for e in sorted(set(rep[d].tolist())):
            if 0 <= e < d and int((sig[e] == sig[d]).sum()) >= min_agree:
                a, b = find(e), find(d)
                parent[max(a, b)] = min(a, b)
    return np.array([find(d) for d in range(n)], dtype=np.int64), rep
