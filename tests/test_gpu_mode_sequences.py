"""Training steps that change the update mode between calls, step by step against the float64 oracle.

aefft_net_step_apply takes (maxdiff, sym) per call and net_step.hip's apply_route() answers each mode with another launch sequence: plain
gradients in operator form take the fused update (taps read through the pending TapUpd, stored by the tail launch), sym or maxdiff take
update(group) + gradient_diff(group), NOGROUP takes the per-pair route.  Every route leaves its own set of caches current for the next step
(planar spectra, the bin-major record, the compact planes, G', the momentum buffers).  Here one net runs a SEQUENCE of modes without being
re-created, and every step is held to the oracle TEACHER-FORCED: np_ref.net_step starts from the weights the GPU itself held before the step
and from the momentum the rule implies (D = w_before - w_after of the step before: exact to half an ulp of w; zero on a fresh net and after
aefft_net_reset_momentum; Df untouched by a tied step, as np_ref.backprop_sym leaves it).  Rounding therefore never accumulates over the
steps and the one-step bounds of test_gpu_fft_path.py / test_gpu_round4.py hold at every step: gradients 5e-5, weights weight_step_tol
(grel 2e-4 where the multiobjective term enters), post-update MSE 2e-4, reconstruction 1e-4.  A gradient evaluated at the weights of one step
earlier -- a cache that a mode change left stale -- is 1e-2 ... 1e-1 away at these shapes.

Net: D = 3, 64 x 64, maps (8, 16, 32), 5 x 5, pool 2, B = 2: the smallest frame at which this net runs as operator_chain with the static
tail; (8, 16, 24) for the generic tail.  Frames are fresh every step, at two amplitudes: floor(U(0, 256)) -- nearly every tap gradient above the
clip knee |g| = 10, so nearly every weight is held to float32 rounding (1e-6) -- and the same frames times 4/256, which straddle the knee.

Sequences of (maxdiff, sym):
  A  (0,0) (1,0) (1,0) (0,0) (0,0)     into and out of the multiobjective route; its buffers allocated in mid-run; momentum built by it
  B  (0,1) (1,1) (1,1) (0,1)           from tied weights
  C  (0,0) (0,1) (0,0) (0,0)           tie in mid-run and untie: the step after uses the Df of step 0
  D  (0,0) (0,0; grad_scale 0.5) reset_momentum (0,0)
  E  (0,0) set_pair(every pair) (0,0)  the new weights, the OLD momentum (include/aefft.h: momentum persists across steps and is reset by
                                       aefft_net_reset_momentum only; aefft_net_set_pair replaces the weights and rebuilds the spectra)

Preconditions asserted on the oracle's side: at amplitude 256 at least 95 % of the tap entries of a step get the 1e-6 bound; at amplitude 4
every pair has 20 ... 95 % of its c gradients below the knee on steps that start from untied weights.  From TIED weights (B, and C after its
tied step) the oracle's pair 0 reconstructs so well at amplitude 4 that all its gradients lie below the knee (pairs 1, 2: 92 ... 96 %); there
the net as a whole is held to have at least 2 % of its tap gradients on either side.
A six-pair net (maps 4,6,4,6,4,6 at 512 x 512, the smallest frame it exists at) runs E: it has no compact planes, so the bin-major record that
aefft_net_set_pair invalidates is rebuilt by the record's own launch, the one reader of the record's pending-update fields outside step_apply.

The other routes (NOCHAIN, NOFUSEUPD, NOGROUP, NOAHEAD, GTAPS, CHAINMSE, NOSTATICCHAIN, set_input_ready) run sequence A without a further
oracle forward: (a) every step's weights against w_before - clip_step(g_used, D_before) in float64, g_used from the route's own packed
gradients and np_ref.gradient_diff_fast -- exact to rounding, so a wrong alpha, a lost grad_scale, a stale D or a wrong weight of the
multiobjective term fail; (b) gradients, MSE and reconstruction of every step against the default route's run.  Both runs are free, so the
bound of (b) is 4 x DRIFT, the distance of the oracle's own float32 replay from its float64 run of the same sequence (measured on the CPU,
np_ref.net_step(dtype=...), this module's weights and frames; the factor is for two float32 routes that sum in different orders):

  step   gradients (relerr, worst segment)   post-update MSE (relative, worst pair)   reconstruction (relerr)
    0              3.6e-07                              7.3e-07                              4.1e-07
    1              7.0e-07                              1.6e-06                              8.2e-07
    2              8.9e-07                              4.1e-07                              1.0e-06
    3              3.9e-06                              5.7e-07                              1.9e-06
    4              8.3e-06                              1.6e-06                              5.0e-06

Routes the library documents as bit-identical to the default (NOSTATICCHAIN, the pipelined mode) are asserted equal."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import np_ref as R
from test_gpu_fft_path import host, relerr, weight_step_tol

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

D, N, NK, POOL, B, DEL0 = 3, 64, 5, 2, 2, 0.2
DELE = 0.1 * DEL0                                   # fft_backproplib.cu:1445
MAPS, MAPS_GENERIC = (8, 16, 32), (8, 16, 24)
S = lambda md, sym, gs=1.0: ("step", md, sym, gs)
SEQS = {  # name: (tied start, operations)
    "A": (False, [S(0, 0), S(1, 0), S(1, 0), S(0, 0), S(0, 0)]),
    "B": (True, [S(0, 1), S(1, 1), S(1, 1), S(0, 1)]),
    "C": (False, [S(0, 0), S(0, 1), S(0, 0), S(0, 0)]),
    "D": (False, [S(0, 0), S(0, 0, 0.5), ("reset",), S(0, 0)]),
    "E": (False, [S(0, 0), ("set_pair",), S(0, 0)]),
}
# the oracle's float32 replay against its float64 run of sequence A at amplitude 256, per step: gradients, MSE, reconstruction (the table above)
DRIFT = [(3.6e-07, 7.3e-07, 4.1e-07), (7.0e-07, 1.6e-06, 8.2e-07), (8.9e-07, 4.1e-07, 1.0e-06), (3.9e-06, 5.7e-07, 1.9e-06),
         (8.3e-06, 1.6e-06, 5.0e-06)]
T = lambda a: np.transpose(a, (1, 0, 2, 3))
f64 = lambda a: np.asarray(a).astype(np.float64)


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context()
    yield c
    c.close()


def _inputs(maps, tied, amp, nframes, size=N):
    """weights U(-1,1) rounded to float32 (a second set for set_pair), fresh frames per step"""
    rng = np.random.default_rng(3 + 100 * maps[-1])
    q32 = lambda a: a.astype(np.float32).astype(np.float64)

    def weights():
        ws, dD = [], D
        for dM in maps:
            c = q32(rng.uniform(-1, 1, (dM, dD, NK, NK)))
            f = q32(rng.uniform(-1, 1, (dD, dM, NK, NK)))
            ws.append((c, q32(rng.uniform(-1, 1, dM)), T(c).copy() if tied else f, q32(rng.uniform(-1, 1, dD)))); dD = dM
        return ws

    ws, ws_new = weights(), weights()
    frames = [np.floor(rng.uniform(0, 256, (B, D, size, size))) * (amp / 256.0) for _ in range(nframes)]
    return ws, ws_new, frames


def _segments(gbuf, ws):
    """the packed buffer's gradient part -> per pair (dck, dfk, db, dp) in float64, and the number of floats taken"""
    out, off = [], 0
    for c, b, f, p in ws:
        nk, dM, dD = c.size, c.shape[0], c.shape[1]
        out.append((f64(gbuf[off:off + nk]).reshape(c.shape), f64(gbuf[off + nk:off + 2 * nk]).reshape(f.shape),
                    f64(gbuf[off + 2 * nk:off + 2 * nk + dM]), f64(gbuf[off + 2 * nk + dM:off + 2 * nk + dM + dD])))
        off += 2 * nk + dM + dD
    return out, off


def _gpu_run(ctx, flags, switches, maps, name, amp, ready=False, size=N):
    """one net through a sequence; per step what the host reads: the packed buffer before and after step_apply, the weights before and after,
    the post-update MSE, the reconstruction.  -> (records, step form, route of the last tail launch)"""
    tied, ops = SEQS[name]
    flags(*switches)
    nsteps = sum(op[0] == "step" for op in ops)
    ws, ws_new, frames = _inputs(maps, tied, amp, nsteps, size)
    L = len(maps)
    net = aefft.Net(ctx, D, size, size, list(maps), NK, POOL, batch=B)
    for l, w in enumerate(ws):
        net.set_pair(l, *w)
    form = net.step_form()
    net.set_input_ready(ready)
    xd = [ctx.dev(x) for x in frames]
    recon, mse = ctx.empty(B, D, size, size), ctx.empty(L)
    ctx.sync()
    w_prev = [tuple(f64(a) for a in net.get_pair(l)) for l in range(L)]
    for l in range(L):
        for a, b in zip(w_prev[l], ws[l]):
            assert np.array_equal(a, b)
    recs, k, event = [], 0, None
    for op in ops:
        if op[0] == "reset":
            net.reset_momentum(); event = "reset"
            continue
        if op[0] == "set_pair":
            for l, w in enumerate(ws_new):
                net.set_pair(l, *w)
            w_prev = [tuple(f64(a) for a in net.get_pair(l)) for l in range(L)]
            for l in range(L):
                for a, b in zip(w_prev[l], ws_new[l]):
                    assert np.array_equal(a, b)
            event = "set_pair"
            continue
        _, md, sym, gs = op
        net.step_grad(xd[k], recon)
        gbuf = host(net.grad_buffer()).copy()
        net.step_apply(DEL0, md, sym, gs, mse)
        ctx.sync()
        w = [tuple(f64(a) for a in net.get_pair(l)) for l in range(L)]
        recs.append(dict(md=md, sym=sym, gs=gs, event=event, xs=frames[k], gbuf=gbuf, gbuf_after=host(net.grad_buffer()).copy(),
                         prev_global=host(net.mse_prev_global()).copy(), mse=host(mse).copy(), recon=host(recon).copy(), w_prev=w_prev, w=w))
        w_prev, event, k = w, None, k + 1
    route = net.tail_route()
    net.close()
    return recs, form, route


def _g_used(grads, w_prev, md, sym, gs):
    """the gradient the rule clips (fft_backproplib.cu:616 behind :657-704; tied: np_ref.backprop_sym): w0*g - w1*g_diff, halved and
    transposed for sym, the reconstruction part times grad_scale.  -> (gc, gf or None, gb, gp)"""
    dck, dfk, db, dp = (gs * g for g in grads)
    if sym:
        gc, gf, gb, gp = 0.5 * (dck + T(dfk)), None, 0.5 * db, 0.5 * dp
    else:
        gc, gf, gb, gp = dck, dfk, db, dp
    if md:
        c, b, f, p = w_prev
        cd, fd, bd, pd = R.gradient_diff_fast(c, f, b, p)
        if sym:
            gc = R.W0 * gc - R.W1 * 0.5 * (cd + T(fd))
        else:
            gc, gf = R.W0 * gc - R.W1 * cd, R.W0 * gf - R.W1 * fd
        gb, gp = R.W0 * gb - R.W1 * bd, R.W0 * gp - R.W1 * pd
    return gc, gf, gb, gp


def _momentum_after(rec, mom):
    """the momentum the device holds after this step, by the rule itself: D = w_before - w_after (w <- w - D); a tied step leaves Df alone"""
    out = []
    for (c0, b0, f0, p0), (c1, b1, f1, p1), m in zip(rec["w_prev"], rec["w"], mom):
        out.append((c0 - c1, m[1] if rec["sym"] else f0 - f1, b0 - b1, p0 - p1))
    return out


def _zero_momentum(ws):
    return [tuple(np.zeros_like(a) for a in (c, f, b, p)) for c, b, f, p in ws]


def _check_buffer(rec, k, prev_mse):
    """the packed buffer around step_apply (include/aefft.h, aefft_net_grad_buffer): the gradient part is read, not written, whatever
    grad_scale is; the tail takes this step's MSE; what stood in the tail -- the previous step's MSE, zero before the first -- is kept, times
    grad_scale, behind the buffer"""
    _, ng = _segments(rec["gbuf"], rec["w"])
    L = len(rec["w"])
    assert rec["gbuf"].size == ng + L
    assert np.array_equal(rec["gbuf"][:ng], rec["gbuf_after"][:ng]), k
    assert np.array_equal(rec["gbuf_after"][ng:], rec["mse"]), k
    assert np.array_equal(rec["gbuf"][ng:], prev_mse), (k, rec["gbuf"][ng:], prev_mse)
    assert np.allclose(rec["prev_global"], prev_mse * np.float32(rec["gs"]), rtol=1e-6, atol=0), (k, rec["prev_global"], prev_mse)


def _check_update_rule(recs):
    """(a): w_k == w_{k-1} - clip_step(g_used, D_{k-1}) in float64 from the route's own packed gradients; no forward"""
    mom, prev_mse = _zero_momentum(recs[0]["w"]), np.zeros(len(recs[0]["w"]), np.float32)
    for k, rec in enumerate(recs):
        if rec["event"] == "reset":
            mom = _zero_momentum(rec["w"])
        md, sym, gs = rec["md"], rec["sym"], rec["gs"]
        grel = 2e-4 if md else 5e-5
        _check_buffer(rec, k, prev_mse)
        grads, _ = _segments(rec["gbuf"], rec["w"])
        for l, (w0, w1, g, m) in enumerate(zip(rec["w_prev"], rec["w"], grads, mom)):
            c0, b0, f0, p0 = w0
            c1, b1, f1, p1 = w1
            gc, gf, gb, gp = _g_used(g, w0, md, sym, gs)
            step = lambda gg, DD: R._clip_step(gg, DD, np.float64(DELE), np.float64)
            for name, got, before, gg, DD in (("c", c1, c0, gc, m[0]), ("f", f1, f0, gf, m[1]), ("b", b1, b0, gb, m[2]), ("p", p1, p0, gp, m[3])):
                if gg is None:
                    continue
                err = np.abs(got - (before - step(gg, DD)))
                assert (err < weight_step_tol(gg, grel=grel)).all(), (k, l, name, err.max())
            if sym:
                assert np.array_equal(f1, T(c1)), (k, l)
            assert np.abs(c1 - c0).max() > 1e-4, (k, l, "the update was not applied")
        mom, prev_mse = _momentum_after(rec, mom), rec["mse"]


def _check_teacher_forced(recs, amp):
    """every step against np_ref.net_step started from the GPU's own weights of the step before and the momentum the rule implies
    (amp: 256 or 4 for the preconditions on this module's nets at those amplitudes, None for none)"""
    mom, L = _zero_momentum(recs[0]["w"]), len(recs[0]["w"])
    for k, rec in enumerate(recs):
        if rec["event"] == "reset":
            mom = _zero_momentum(rec["w"])
        md, sym, gs = rec["md"], rec["sym"], rec["gs"]
        grel = 2e-4 if md else 5e-5
        ws2, _, mses, recon, grads = R.net_step(rec["xs"], rec["w_prev"], mom, POOL, DEL0, md, sym, grad_scale=gs, return_grads=True)
        got_g, _ = _segments(rec["gbuf"], rec["w"])
        assert relerr(rec["recon"], recon) < 1e-4, (k, relerr(rec["recon"], recon))
        tight = total = n_below = n_taps = 0
        for l in range(L):
            for i, (seg, ref) in enumerate(zip(got_g[l], grads[l])):
                e = relerr(seg, ref)
                print(f"step {k} pair {l} segment {i}: gradient relerr {e:.2e}")
                assert e < 5e-5, (k, l, i, e)
            below = float(np.mean(np.abs(grads[l][0]) < 10.0))
            print(f"step {k} pair {l}: share of c's gradients below the knee {below:.3f}")
            # amplitude 4: both branches of clip_step and their seam in every pair.  (From tied weights, f == c^T, the oracle's pair 0
            # reconstructs so well that ALL its gradients lie below the knee, and 92 ... 96 % of the other pairs': there the whole net is
            # held to have at least 2 % of its tap gradients on either side.)
            tied = np.array_equal(rec["w_prev"][l][2], T(rec["w_prev"][l][0]))
            n_below += int((np.abs(grads[l][0]) < 10.0).sum()); n_taps += grads[l][0].size
            if amp == 4 and not tied:
                assert 0.20 <= below <= 0.95, (k, l, below)
            if amp == 4 and tied and l == L - 1:
                assert 0.02 <= n_below / n_taps <= 0.98, (k, n_below, n_taps)
            c1, b1, f1, p1 = rec["w"][l]
            rc, rb, rf, rp = ws2[l]
            gc, gf, gb, gp = _g_used(grads[l], rec["w_prev"][l], md, sym, gs)
            for name, got, ref, gg in (("c", c1, rc, gc), ("f", f1, rf, gf), ("b", b1, rb, gb), ("p", p1, rp, gp)):
                if gg is None:
                    continue
                tol = weight_step_tol(gg, grel=grel)
                err = np.abs(got - ref)
                print(f"step {k} pair {l} {name}: worst weight error {err.max():.2e}, worst error / bound {(err / tol).max():.3f}")
                assert (err < tol).all(), (k, l, name, err.max())
                if name in "cf":
                    tight += int((tol == 1e-6).sum()); total += tol.size
            if sym:
                assert np.array_equal(f1, T(c1)), (k, l)
            assert np.abs(c1 - rec["w_prev"][l][0]).max() > 1e-4, (k, l, "the update was not applied")
            print(f"step {k} pair {l}: post-update MSE {rec['mse'][l]:.6e}, oracle {mses[l]:.6e}")
            assert abs(rec["mse"][l] - mses[l]) < 2e-4 * mses[l], (k, l, rec["mse"][l], mses[l])
        print(f"step {k}: {tight / total:.4f} of the tap entries held to 1e-6")
        if amp == 256:
            assert tight >= 0.95 * total, (k, tight, total)       # the comparison is exact to float32 rounding where it matters
        mom = _momentum_after(rec, mom)


# default form: every sequence at both amplitudes; per-frame form: every sequence, the amplitudes alternating (some 60 oracle steps in all)
CASES = [("", s, a) for s in "ABCDE" for a in (256, 4)] + [("NOOPFORM", s, a) for s, a in zip("ABCDE", (256, 4, 256, 4, 4))]


@pytest.mark.parametrize("path,name,amp", CASES)
def test_mode_sequence_teacher_forced_against_the_oracle(ctx, flags, path, name, amp):
    recs, form, route = _gpu_run(ctx, flags, [path], MAPS, name, amp)
    assert form == ("per_frame" if path else "operator_chain")
    if not path:
        assert route == "static"
    _check_update_rule(recs)
    _check_teacher_forced(recs, amp)


def test_mode_sequence_on_the_generic_tail_against_the_oracle(ctx, flags):
    recs, form, route = _gpu_run(ctx, flags, [], MAPS_GENERIC, "A", 256)
    assert (form, route) == ("operator_chain", "generic")
    _check_update_rule(recs)
    _check_teacher_forced(recs, 256)


def test_set_pair_after_a_fused_step_on_a_net_without_compact_planes(ctx, flags):
    """Six pairs: the compact planes Cc_l exist for up to five, so here the bin-major record that aefft_net_set_pair invalidates is rebuilt
    by the record's own launch (kspec_packed), which reads the taps through the record's update fields -- after a fused step these must have
    been cleared, or the new weights enter the chain with the last step's update applied once more.  512 x 512 is the smallest frame at
    which six pool-2 pairs exist (innermost grid 8 x 8).  Sequence E, teacher-forced."""
    recs, form, _ = _gpu_run(ctx, flags, [], (4, 6, 4, 6, 4, 6), "E", 256, size=512)
    assert form in ("operator", "operator_chain")
    _check_update_rule(recs)
    _check_teacher_forced(recs, None)


_default = {}


def _default_run(ctx, flags):
    """the default route's free run of sequence A at amplitude 256: computed once, left unchanged"""
    if not _default:
        recs, form, route = _gpu_run(ctx, flags, [], MAPS, "A", 256)
        assert (form, route) == ("operator_chain", "static")
        _default["recs"] = recs
    return _default["recs"]


ROUTES = {  # name: (development switches, set_input_ready, documented as bit-identical to the default route)
    "NOCHAIN": (["NOCHAIN"], False, False), "NOFUSEUPD": (["NOFUSEUPD"], False, False), "NOGROUP": (["NOGROUP"], False, False),
    "NOAHEAD": (["NOAHEAD"], False, False), "GTAPS": (["GTAPS"], False, False), "CHAINMSE": (["CHAINMSE"], False, False),
    "NOSTATICCHAIN": (["NOSTATICCHAIN"], False, True), "input_ready": ([], True, True),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_other_routes_through_sequence_A(ctx, flags, route):
    switches, ready, same_bits = ROUTES[route]
    want = _default_run(ctx, flags)
    recs, form, tail = _gpu_run(ctx, flags, switches, MAPS, "A", 256, ready=ready)
    if route == "NOSTATICCHAIN":
        assert (form, tail) == ("operator_chain", "generic")
    _check_update_rule(recs)
    assert len(recs) == len(want) == len(DRIFT)
    for k, (a, b, (dg, dm, dr)) in enumerate(zip(recs, want, DRIFT)):
        if same_bits:
            for key in ("gbuf", "gbuf_after", "mse", "recon"):
                assert np.array_equal(a[key], b[key]), (k, key)
            for wa, wb in zip(a["w"], b["w"]):
                for u, v in zip(wa, wb):
                    assert np.array_equal(u, v), k
            continue
        ga, ng = _segments(a["gbuf"], a["w"])
        gb, _ = _segments(b["gbuf"], b["w"])
        eg = max(relerr(x, y) for pa, pb in zip(ga, gb) for x, y in zip(pa, pb))
        em = float(np.abs(f64(a["mse"]) / f64(b["mse"]) - 1).max())
        er = relerr(a["recon"], b["recon"])
        print(f"step {k}: against the default route: gradients {eg:.2e} (bound {4 * dg:.1e}), MSE {em:.2e} ({4 * dm:.1e}), reconstruction {er:.2e} ({4 * dr:.1e})")
        assert eg < 4 * dg and em < 4 * dm and er < 4 * dr, (k, eg, em, er)
