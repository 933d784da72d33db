"""aefft_map_stats_update / _merge / _finish and aefft_map_peak restated in numpy from include/aefft.h alone, for the tests: sequential float64
additions in ascending b, a sort for the extremes, the finish formulas line by line (numpy's float64 operations round once each and never fuse; its
sqrt is correctly rounded), the peak by argmax on a NaN-masked copy.  A state is a dict of the five planes -- S1, S2 float64 [n], hi, lo float32
[4][n] with the dead slots already +0, c int32 [n] --; to_bytes gives the bytes of the device layout.  No function changes its arguments.  The product
never imports this module."""
import numpy as np

MODES = {"sigma": 0, "rank": 1}
SENSES = {"above": 0, "below": 1}
QNAN = np.uint32(0x7FC00000)


def stats_bytes(Mx, My):
    return (52 * Mx * My + 15) // 16 * 16 if 1 <= Mx <= 1024 and 1 <= My <= 1024 else 0


def empty(Mx, My):
    n = Mx * My
    return dict(S1=np.zeros(n), S2=np.zeros(n), hi=np.zeros((4, n), np.float32), lo=np.zeros((4, n), np.float32), c=np.zeros(n, np.int32))


def _live(state):
    """hi and lo with the dead slots at -inf and +inf"""
    dead = np.arange(4)[:, None] >= state["c"][None, :]
    return np.where(dead, np.float32(-np.inf), state["hi"]), np.where(dead, np.float32(np.inf), state["lo"])


def _dead_to_zero(hi, lo, c):
    dead = np.arange(4)[:, None] >= c[None, :]
    return np.where(dead, np.float32(0), hi).astype(np.float32), np.where(dead, np.float32(0), lo).astype(np.float32)


def update(state, maps):
    """the maps [B][Mx][My] (float32) enter the state, b ascending"""
    maps = np.asarray(maps, np.float32)
    S1, S2, c = state["S1"].copy(), state["S2"].copy(), state["c"].copy()
    hi, lo = _live(state)
    for b in range(maps.shape[0]):
        x = maps[b].reshape(-1).copy()
        ok = np.isfinite(x)
        x[x == 0] = 0.0                                                          # -0 counts as +0
        d = np.where(ok, x, 0).astype(np.float64)
        S1 = np.where(ok, S1 + d, S1)
        S2 = np.where(ok, S2 + d * d, S2)                                        # (the product is exact)
        c = c + ok.astype(np.int32)
        hi = -np.sort(-np.concatenate([hi, np.where(ok, x, np.float32(-np.inf))[None]]), axis=0)[:4]
        lo = np.sort(np.concatenate([lo, np.where(ok, x, np.float32(np.inf))[None]]), axis=0)[:4]
    hi, lo = _dead_to_zero(hi, lo, c)
    return dict(S1=S1, S2=S2, hi=hi, lo=lo, c=c)


def merge(dst, src):
    c = dst["c"] + src["c"]
    dh, dl = _live(dst)
    sh, sl = _live(src)
    hi = -np.sort(-np.concatenate([dh, sh]), axis=0)[:4]
    lo = np.sort(np.concatenate([dl, sl]), axis=0)[:4]
    hi, lo = _dead_to_zero(hi, lo, c)
    return dict(S1=dst["S1"] + src["S1"], S2=dst["S2"] + src["S2"], hi=hi, lo=lo, c=c.astype(np.int32))


def to_bytes(state, Mx, My):
    n = Mx * My
    out = np.zeros(stats_bytes(Mx, My), np.uint8)
    out[:8 * n] = state["S1"].astype("<f8").view(np.uint8)
    out[8 * n:16 * n] = state["S2"].astype("<f8").view(np.uint8)
    out[16 * n:32 * n] = np.ascontiguousarray(state["hi"], "<f4").reshape(-1).view(np.uint8)
    out[32 * n:48 * n] = np.ascontiguousarray(state["lo"], "<f4").reshape(-1).view(np.uint8)
    out[48 * n:52 * n] = state["c"].astype("<i4").view(np.uint8)
    return out


def from_bytes(buf, Mx, My):
    n = Mx * My
    b = np.ascontiguousarray(buf, np.uint8)
    return dict(S1=b[:8 * n].view("<f8").copy(), S2=b[8 * n:16 * n].view("<f8").copy(), hi=b[16 * n:32 * n].view("<f4").reshape(4, n).copy(),
                lo=b[32 * n:48 * n].view("<f4").reshape(4, n).copy(), c=b[48 * n:52 * n].view("<i4").copy())


def finish(state, Mx, My, mode="rank", sense="above", k=3.0, rank=1, empty=np.inf):
    """ref, float32 [Mx][My]"""
    c = state["c"]
    n = c.size
    if mode == "rank":
        r = np.minimum(rank, c)
        slots = state["lo"] if sense == "below" else state["hi"]
        ref = slots[np.maximum(r - 1, 0), np.arange(n)]
    else:
        with np.errstate(all="ignore"):
            S1, S2 = state["S1"], state["S2"]
            cd = c.astype(np.float64)
            mean = S1 / cd
            p = S1 * mean
            d = S2 - p
            d = np.where(d < 0, 0.0, d)
            var = d / (cd - 1.0)
            sd = np.where(c == 1, 0.0, np.sqrt(var))
            t = np.float64(np.float32(k)) * sd
            ref = (mean + t).astype(np.float32)
    return np.where(c == 0, np.float32(empty), ref).astype(np.float32).reshape(Mx, My)


def peak(maps, ref=None, sense="above"):
    """(peak float32 [B], cell int32 [B]) of the maps [B][Mx][My]"""
    maps = np.asarray(maps, np.float32)
    B = maps.shape[0]
    pk, cell = np.zeros(B, np.float32), np.zeros(B, np.int32)
    for b in range(B):
        with np.errstate(all="ignore"):
            v = (maps[b] if ref is None else maps[b] - np.asarray(ref, np.float32)).astype(np.float32).reshape(-1).copy()
        v[v == 0] = 0.0
        nan = np.isnan(v)
        if nan.all():
            pk[b:b + 1].view(np.uint32)[0] = QNAN
            cell[b] = -1
            continue
        masked = np.where(nan, np.float32(np.inf if sense == "below" else -np.inf), v)
        best = masked.min() if sense == "below" else masked.max()
        cell[b] = np.argmax(~nan & (v == best))                                  # the smallest index that attains it
        pk[b] = v[cell[b]]
    return pk, cell
