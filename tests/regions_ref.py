"""aefft_map_regions restated (include/aefft.h "aefft_map_regions", steps 1-7) in numpy and plain Python: an iterative flood fill in scan order.  It
shares nothing with the kernels -- no union-find, no keys, no tiles.  The float32 subtraction goes through numpy; everything else is comparisons
and integers, so labels, counts and region bytes are defined exactly.  A plain module: pytest collects nothing from it."""
import numpy as np

REGION = np.dtype([("i0", "<i4"), ("j0", "<i4"), ("i1", "<i4"), ("j1", "<i4"), ("area", "<i4"), ("peak_i", "<i4"), ("peak_j", "<i4"), ("peak", "<f4")])
assert REGION.itemsize == 32
NEIGHBOURS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)), 8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def values(map, ref=None):
    """step 1: v = map, or map - ref rounded once to float32; a -0 result counts as +0"""
    m = np.asarray(map, np.float32)
    with np.errstate(invalid="ignore"):
        v = m.copy() if ref is None else (m - np.asarray(ref, np.float32)[None]).astype(np.float32)
    v[v == 0] = np.float32(0.0)
    return v


def foreground(v, sense, lo, hi):
    """step 2: (foreground, strong); NaN compares false"""
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(invalid="ignore"):
        return (v >= lo, v >= hi) if sense == "above" else (v <= lo, v <= hi)


def components(fg, connectivity):
    """step 3: the components of one image's mask [Mx][My] as lists of linear indices, in ascending order of their smallest index"""
    Mx, My = fg.shape
    seen = np.zeros(Mx * My, bool)
    flat = fg.reshape(-1)
    out = []
    for p in np.flatnonzero(flat):
        if seen[p]:
            continue
        seen[p] = True
        comp, stack = [], [int(p)]
        while stack:
            q = stack.pop()
            comp.append(q)
            I, J = divmod(q, My)
            for di, dj in NEIGHBOURS[connectivity]:
                a, c = I + di, J + dj
                if 0 <= a < Mx and 0 <= c < My:
                    n = a * My + c
                    if flat[n] and not seen[n]:
                        seen[n] = True
                        stack.append(n)
        out.append(comp)
    return out


def regions(map, lo, hi=None, ref=None, sense="above", connectivity=8, min_area=1, max_regions=256, fill=None):
    """(labels int32 [B][Mx][My], regions REGION [B][max_regions], count int32 [B]); `fill`: what the regions array holds beforehand (the entries
    from min(n, max_regions) on keep it), zeros when None"""
    hi = lo if hi is None else hi
    assert sense in ("above", "below") and connectivity in (4, 8) and min_area >= 1
    assert (lo <= hi) if sense == "above" else (hi <= lo)
    v = values(map, ref)
    B, Mx, My = v.shape
    fg, strong = foreground(v, sense, lo, hi)
    labels = np.zeros((B, Mx, My), np.int32)
    count = np.zeros(B, np.int32)
    out = np.zeros((B, max_regions), REGION) if fill is None else np.array(fill, REGION).reshape(B, max_regions).copy()
    for b in range(B):
        vb, sb, lb = v[b].reshape(-1), strong[b].reshape(-1), labels[b].reshape(-1)
        n = 0
        for comp in components(fg[b], connectivity):
            c = np.array(comp)
            if not sb[c].any() or len(comp) < min_area:                     # step 4
                continue
            n += 1                                                            # step 5: scan order is the order of the smallest index
            lb[c] = n
            if n <= max_regions:                                              # step 6
                I, J = c // My, c % My
                best = vb[c].max() if sense == "above" else vb[c].min()
                peak = int(c[vb[c] == best].min())                            # the smallest index that attains it
                out[b, n - 1] = (I.min(), J.min(), I.max(), J.max(), len(comp), peak // My, peak % My, best)
        count[b] = n
    return labels, out, count


def to_pixels(r, Mx, My, W, H):
    """step 7: the half-open pixel box (x0, y0, x1, y1) of a region's inclusive cell bounds"""
    ceil = lambda a, b: -(-a // b)
    return ceil(int(r["i0"]) * W, Mx), ceil(int(r["j0"]) * H, My), ceil((int(r["i1"]) + 1) * W, Mx), ceil((int(r["j1"]) + 1) * H, My)


# ---- the patterns of the tests: boolean masks [Mx][My] -----------------------------------------
def spiral(Mx, My):
    """a track one cell wide that winds inwards with a gap of one cell: it crosses every tile and gives long chains"""
    m = np.zeros((Mx, My), bool)
    i = j = di = 0
    dj, turned = 1, 0
    m[0, 0] = True
    inside = lambda a, c: 0 <= a < Mx and 0 <= c < My
    while turned < 2:
        ni, nj = i + di, j + dj
        if inside(ni, nj) and not m[ni, nj] and not (inside(ni + di, nj + dj) and m[ni + di, nj + dj]):
            i, j, turned = ni, nj, 0
            m[i, j] = True
        else:
            di, dj, turned = dj, -di, turned + 1
    return m


def pattern(kind, Mx, My, rng=None):
    I, J = np.indices((Mx, My))
    if kind == "empty":
        return np.zeros((Mx, My), bool)
    if kind == "full":
        return np.ones((Mx, My), bool)
    if kind == "spiral":
        return spiral(Mx, My)
    if kind == "u":
        return (J == 0) | (J == My - 1) | (I == Mx - 1)                       # the arms meet at the far end
    if kind == "comb":
        return (I == Mx - 1) | (J % 2 == 0)                                   # teeth along I, joined by the last row
    if kind == "ring":
        return (I == 0) | (I == Mx - 1) | (J == 0) | (J == My - 1) | ((I == Mx // 2) & (J == My // 2) & (Mx > 4) & (My > 4))
    if kind == "diag":
        return (I % My == J) | (J % Mx == I)
    if kind == "antidiag":
        return (I + J) % max(Mx, My) == max(Mx, My) - 1
    if kind == "checker":
        return (I + J) % 2 == 0
    if kind == "bars":
        return (I % 3 == 0) | (J % 19 == 5)                                   # components across every tile in both directions
    if kind.startswith("random"):
        return rng.random((Mx, My)) < float(kind[6:]) / 100.0
    raise ValueError(kind)
