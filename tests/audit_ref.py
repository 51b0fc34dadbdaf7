"""A restatement of the audit's host rules (cough_detector_amd/audit.py) in plain Python loops over float64, written from
the rules' text and not from that module: the fold assignment of ``stratified_kfold`` and the confident-learning rule of
``find_label_issues``.  Also the synthetic audit corpus' seeds and planted flips, which the GPU test and the recorded
reference run (tests/golden/audit_synth.json) share."""
import math

import numpy as np


def kfold(labels, folds=5, random_state=42):
    """Deal each class's permuted members round the folds; class 1 goes on where class 0 stopped."""
    labels = [int(v) for v in labels]
    rng = np.random.RandomState(random_state)
    out = [-1] * len(labels)
    start = 0
    for c in (0, 1):
        members = np.array([i for i, v in enumerate(labels) if v == c], dtype=np.int64)
        order = rng.permutation(members)
        for m, i in enumerate(order):
            out[int(i)] = (m + start) % folds
        start = (start + len(order)) % folds
    return np.array(out, dtype=np.int64)


def label_issues(prob, labels):
    """-> dict(thresholds, suggested, margin, self_confidence, suspects, ranking, unscored, noise_rate).  A row with a
    NaN is unscored: it does not enter the threshold means, is never a suspect and is not ranked."""
    p = [[float(a), float(b)] for a, b in np.asarray(prob, dtype=np.float64)]
    y = [int(v) for v in labels]
    n = len(y)
    unscored = [i for i in range(n) if math.isnan(p[i][0]) or math.isnan(p[i][1])]
    scored = [i for i in range(n) if i not in set(unscored)]
    t = []
    for j in (0, 1):
        mine = [p[i][j] for i in scored if y[i] == j]
        t.append(float(np.mean(np.array(mine, dtype=np.float64))) if mine else float("nan"))
    suggested, margin, conf = list(y), [float("nan")] * n, [float("nan")] * n
    for i in scored:
        c = [j for j in (0, 1) if p[i][j] >= t[j]]
        if len(c) == 1:
            suggested[i] = c[0]
        elif len(c) == 2 and p[i][0] != p[i][1]:
            suggested[i] = 0 if p[i][0] > p[i][1] else 1
        margin[i] = p[i][y[i]] - p[i][1 - y[i]]
        conf[i] = p[i][y[i]]
    ranking = sorted(scored, key=lambda i: (margin[i], i))
    suspects = [i for i in ranking if suggested[i] != y[i]]
    noise = {}
    for j in (0, 1):
        count = sum(1 for v in y if v == j)
        noise[j] = sum(1 for i in suspects if y[i] == j) / count if count else float("nan")
    return dict(thresholds=t, suggested=suggested, margin=margin, self_confidence=conf, suspects=suspects,
                ranking=ranking, unscored=unscored, noise_rate=noise)


# ------------------------------------------------------------------------------------------------ the synthetic corpus
N_NON_COUGH, N_COUGH, N_FLIPS_PER_CLASS = 120, 60, 6


def synth_corpus():
    """-> (seeds, true labels, given labels, planted): 180 ``synth.make_clip`` seeds, non-cough first -- the first 120
    seeds >= 1 that are no multiple of 6, then ``6 * j`` for j < 60 (``seed % 6 == 0`` is the cough-like kind) -- and
    12 labels flipped, 6 per class, drawn without replacement from ``np.random.RandomState(0)``: first among the
    non-cough clips, then among the cough clips.  ``planted``: the flipped indices, ascending."""
    seeds = [s for s in range(1, 1000) if s % 6][:N_NON_COUGH] + [6 * j for j in range(N_COUGH)]
    true = np.array([0] * N_NON_COUGH + [1] * N_COUGH, dtype=np.int64)
    rng = np.random.RandomState(0)
    planted = np.sort(np.concatenate([rng.choice(N_NON_COUGH, N_FLIPS_PER_CLASS, replace=False),
                                      N_NON_COUGH + rng.choice(N_COUGH, N_FLIPS_PER_CLASS, replace=False)]))
    given = true.copy()
    given[planted] = 1 - given[planted]
    return seeds, true, given, planted
