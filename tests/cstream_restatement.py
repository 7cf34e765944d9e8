"""A numpy restatement of the streamed frequency tables (fg_diag_cstream): per watched row np.bincount of cells - lo inside
[lo, lo + bins), the counts below and above, and the smallest and largest cell; FG_U64 rows compare as unsigned, the other integer
tags as signed.  Python integers where a value may pass 2^63.  Shared by tests/test_diag_cstream_cpu.py and
tests/test_gpu_diag_cstream.py, with the mixed input both feed."""
import numpy as np

FG_F64, FG_BOOL, FG_U64, FG_USIZE, FG_I64 = range(5)
FG_E_BAD_ARG, FG_E_STATE = -3, -5
CHUNKINGS = ([97], [5, 31, 1, 60], [1] * 97)


def tabulate_row(cells, vtype, lo, bins):
    """cells: int64 array of any shape (the 8-byte cells of one row) -> dict(counts uint64 [bins], below, above, min, max)."""
    v = np.ascontiguousarray(cells).reshape(-1)
    v = v.view(np.uint64) if vtype == FG_U64 else v.view(np.int64)
    lo = int(lo)
    if vtype == FG_U64:
        lo_t, hi = np.uint64(lo), lo + bins                        # hi as a Python integer: it may be 2^64
        below = v < lo_t
        above = np.array([int(x) >= hi for x in v]) if hi >= 2 ** 64 else v >= np.uint64(hi)
    else:
        below = v < np.int64(lo)
        above = v > np.int64(lo + bins - 1)
    inside = ~(below | above)
    off = (v[inside] - (np.uint64(lo) if vtype == FG_U64 else np.int64(lo))).astype(np.int64)
    return dict(counts=np.bincount(off, minlength=bins).astype(np.uint64), below=int(below.sum()), above=int(above.sum()),
                min=int(v.min()), max=int(v.max()))


def tabulate(cells, rows, vtypes, lo, bins):
    """cells [n][n_rec][C] int64 -> one tabulate_row per watched row."""
    return [tabulate_row(cells[:, r, :], vt, l, b) for r, vt, l, b in zip(rows, vtypes, lo, bins)]


def same_tables(got, want):
    """got / want: lists of dict(counts, below, above, min, max)."""
    return len(got) == len(want) and all(
        np.array_equal(np.asarray(g["counts"], dtype=np.uint64), np.asarray(w["counts"], dtype=np.uint64)) and
        all(int(g[k]) == int(w[k]) for k in ("below", "above", "min", "max")) for g, w in zip(got, want))


def mixed_input(n=97, C=70, seed=11):
    """cells [n][5][C]: an f64 row (not watched), a bool row, a usize row with K = 4, an i64 row with values on both sides of
    [-3, 6), a u64 row that holds 2^63 + 5.  -> (cells int64, watch = dict(rows, vtypes, lo, bins))."""
    rng = np.random.default_rng(seed)
    cells = np.zeros((n, 5, C), dtype=np.int64)
    cells[:, 0, :] = rng.standard_normal((n, C)).view(np.int64)
    cells[:, 1, :] = rng.integers(0, 2, size=(n, C))
    cells[:, 2, :] = rng.integers(0, 4, size=(n, C))
    cells[:, 3, :] = rng.integers(-9, 12, size=(n, C))
    u = rng.integers(0, 11, size=(n, C)).astype(np.uint64)
    u[min(3, n - 1), min(7, C - 1)] = np.uint64(2 ** 63 + 5)
    u[n - 1, C - 1] = np.uint64(2 ** 63 + 5)
    cells[:, 4, :] = u.view(np.int64)
    return cells, dict(rows=[1, 2, 3, 4], vtypes=[FG_BOOL, FG_USIZE, FG_I64, FG_U64], lo=[0, 0, -3, 0], bins=[2, 4, 9, 8])


def show(label, tables):
    for k, t in enumerate(tables):
        print(f"{label} row {k}: counts {np.asarray(t['counts']).tolist()} below {int(t['below'])} above {int(t['above'])} min {int(t['min'])} max {int(t['max'])}")
