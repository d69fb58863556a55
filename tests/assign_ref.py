"""A plain numpy restatement of the device solver of include/umereg_assign.h (csrc/assign.hip): shortest augmenting paths with fp64
duals over fp32 costs, the same start (row minima; column minima of the reduced matrix when the matrix is square; rounds of
"every free row names its lowest free zero, a column takes the lowest row that named it") and the lowest index on ties.  Written
from the scheme, not from scipy's source; tests compare it WITH scipy."""
import numpy as np

START_ROUNDS = 2        # UMEREG_ASSIGN_START_ROUNDS


def linear_sum_assignment_ref(cost, stats=None):
    """cost [n, m] with n <= m (converted to float32, as the device reads it) -> (rows, cols, total): rows = arange(n), cols int64
    [n], total = the fp64 sum of the chosen costs in row order.  stats: a dict that receives `matched` (rows matched by the start)
    and `steps` (Dijkstra steps)."""
    c = np.asarray(cost, dtype=np.float32).astype(np.float64)
    n, m = c.shape
    assert 0 < n <= m and np.isfinite(c).all()
    u = c.min(axis=1)
    v = (c - u[:, None]).min(axis=0) if n == m else np.zeros(m)
    col4row = np.full(n, -1, dtype=np.int64)
    row4col = np.full(m, -1, dtype=np.int64)
    for _ in range(START_ROUNDS):
        claim = {}
        for i in np.flatnonzero(col4row < 0):
            zero = np.flatnonzero((((c[i] - u[i]) - v) == 0.0) & (row4col < 0))
            if len(zero):
                claim.setdefault(int(zero[0]), int(i))      # rows ascend: the first to name a column is the lowest
        for j, i in claim.items():
            col4row[i], row4col[j] = j, i
    free = np.flatnonzero(col4row < 0)
    steps = 0
    for cur in free:
        shortest = np.full(m, np.inf)
        pred = np.full(m, -1, dtype=np.int64)
        visited = np.zeros(m, dtype=bool)
        i, min_val, sink = int(cur), 0.0, -1
        for _ in range(m):
            r = ((min_val + c[i]) - u[i]) - v
            better = ~visited & (r < shortest)
            shortest[better] = r[better]
            pred[better] = i
            cand = np.where(visited, np.inf, shortest)
            j = int(np.argmin(cand))                          # the first of equal minima
            if visited[j]:                                    # (every unvisited column at infinity: not with finite costs)
                j = int(np.flatnonzero(~visited)[0])
            steps += 1
            min_val = shortest[j]
            visited[j] = True
            if row4col[j] < 0:
                sink = j
                break
            i = int(row4col[j])
        assert sink >= 0
        d = min_val - shortest[visited]
        others = visited.copy()
        others[sink] = False
        u[row4col[others]] += min_val - shortest[others]
        u[cur] += min_val
        v[visited] -= d
        j = sink
        while True:
            i = int(pred[j])
            row4col[j] = i
            j, col4row[i] = int(col4row[i]), j
            if i == cur:
                break
    total = 0.0
    for i in range(n):
        total += c[i, col4row[i]]
    if stats is not None:
        stats.update(matched=n - len(free), steps=steps)
    return np.arange(n, dtype=np.int64), col4row.copy(), total
