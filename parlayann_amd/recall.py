"""Tie-aware recall, as checkRecall computes it (algorithms/utils/check_nn_recall.h:83-109):
the first k ground-truth ids plus every later ground-truth entry whose distance equals the k-th
distance form the accepted set; each accepted id found among the k reported ids counts once; the
sum is divided by k * nq."""
import numpy as np


def recall_at_k(result_ids, gt_ids, gt_dists, k):
    result_ids = np.asarray(result_ids)[:, :k]
    gt_ids = np.asarray(gt_ids)
    gt_dists = np.asarray(gt_dists)
    nq = len(result_ids)
    accept = np.zeros(gt_ids.shape, dtype=bool)
    accept[:, :k] = True
    accept[:, k:] = gt_dists[:, k:] == gt_dists[:, k - 1:k]
    hits = 0
    for i in range(nq):
        hits += int(np.isin(gt_ids[i][accept[i]], result_ids[i]).sum())
    return hits / float(k * nq)


def range_recall(result_ids, result_counts, gt_offsets, gt_ids):
    """checkRangeRecall (algorithms/utils/check_range_recall.h:37-53) for range-search results against a range ground truth
    (CSR: gt_offsets n + 1 entries, gt_ids).  The reference divides result COUNTS ("since distances are exact"); here a hit is
    an id in |reported ∩ truth|, which is the same number whenever every reported id is a true match and can never exceed 1.
      pointwise  : mean over the queries with a non-empty truth of hits / truth size
      cumulative : all hits / all truth entries
    -> dict(pointwise, cumulative, reported, total, nonzero); a ratio with an empty denominator is NaN (0 / 0 upstream)."""
    result_ids = np.asarray(result_ids)
    result_counts = np.asarray(result_counts).astype(np.int64)
    gt_offsets = np.asarray(gt_offsets).astype(np.int64)
    gt_ids = np.asarray(gt_ids)
    nq = len(result_counts)
    if len(gt_offsets) != nq + 1:
        raise ValueError(f"{nq} result rows, ground truth of {len(gt_offsets) - 1} queries")
    pointwise = 0.0
    hits_all = reported = nonzero = 0
    for i in range(nq):
        rep = np.unique(result_ids[i, : result_counts[i]])
        truth = gt_ids[gt_offsets[i]: gt_offsets[i + 1]]
        reported += len(rep)
        if len(truth):
            hits = int(np.isin(rep, truth).sum())
            hits_all += hits
            pointwise += hits / float(len(truth))
            nonzero += 1
    total = int(gt_offsets[nq])
    return {"pointwise": pointwise / nonzero if nonzero else float("nan"),
            "cumulative": hits_all / float(total) if total else float("nan"),
            "reported": int(reported), "total": total, "nonzero": int(nonzero)}
