"""The numpy restatement of gpe_query_clusters (include/gpe.h): the pairs of tests/_contacts_model.contacts (the
binary32 predicate, brute force over all pairs), then minimum-label propagation along them to a fixed point -- every
particle ends with the lowest storage index its contacts can reach.  Integers only: nothing to round, no order to
depend on."""
import numpy as np

from tests._contacts_model import contacts

U32 = np.uint32


def labels_from_pairs(n, a, b):
    """label u32[n]: the lowest index of each connected component of the graph with the edges (a[k], b[k])"""
    label = np.arange(n, dtype=np.int64)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    while True:
        before = label.copy()
        low = np.minimum(label[a], label[b])
        np.minimum.at(label, a, low)
        np.minimum.at(label, b, low)
        label = label[label]                                # jump: a label's own label is at most as large
        if np.array_equal(label, before):
            return label.astype(U32)


def summary(label):
    """(size u32[n], count, largest_size, largest_label) of a label array; (.., 0, 0, 0) without particles"""
    n = label.shape[0]
    if n == 0:
        return np.zeros(0, U32), 0, 0, 0
    per_root = np.bincount(label, minlength=n)
    size = per_root[label].astype(U32)
    count = int(np.count_nonzero(label == np.arange(n)))
    largest_size = int(per_root.max())
    largest_label = int(np.flatnonzero(per_root == largest_size)[0])       # the lowest label of that size
    return size, count, largest_size, largest_label


def clusters(pos, rad):
    """-> (label u32[n], size u32[n], count, largest_size, largest_label)"""
    n = len(np.ascontiguousarray(rad).reshape(-1))
    _, _, a, b, _ = contacts(pos, rad)
    label = labels_from_pairs(n, a, b)
    return (label,) + summary(label)
