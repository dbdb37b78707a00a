"""The closure consistency gate on the device (pr_gate, gate.hip) against the NumPy restatement (gate_np.py).

Equality is of BYTES throughout - keep, support, map, info, the rows of dst and dst.state: the rule needs only + and x in fp64, the
kernels are built without contraction, and the only atomics are integer adds.  No decision of a noisy case hangs on a rounding
(test_gate_cpu.py: every comparable pair is at least 1e-6, relatively, from its table entry), and the threshold cases are exact
arithmetic.  Guard words stand behind every output and guard rows in dst behind `kept`.

The outlier case, measured on an MI355X (largest |pose entry - ground truth| over the 40 nodes): input 0.565, ungated relaxation 31.7,
gated relaxation 0.351; only the order of the last two is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import gate_np as gn
import posegraph_np as pg
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import _stream_context

pytestmark = pytest.mark.gpu

GUARD = -7
GUARD8 = 249
NAMES = api.PoseGraph.NAMES


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def load_src(g, log):
    """the model's four buffers as they are (an add would refuse the invalid edges the gate has to skip)"""
    g.edge_ij.copy_(dev(log.edge_ij, np.int32)); g.edge_Z.copy_(dev(log.edge_Z)); g.edge_w.copy_(dev(log.edge_w)); g.state.copy_(dev(log.state, np.int32))


class Rig:
    """a source graph holding the case's log, a destination graph over guarded buffers filled with the guard pattern, the gate, and
    guarded outputs"""

    def __init__(self, case, dst_cap=None):
        self.ctx = _stream_context(0)
        self.case, self.NC, self.EC = case, case["node_capacity"], case["cap"]
        self.DC = dst_cap or self.EC
        DC, EC, NC = self.DC, self.EC, self.NC
        self.src = api.PoseGraph(self.ctx, NC, EC)
        self.big = dict(edge_ij=torch.zeros((DC + 1, 2), dtype=torch.int32, device="cuda"), edge_Z=torch.zeros((DC + 1, 12), dtype=torch.float64, device="cuda"),
                        edge_w=torch.zeros((DC + 1, 2), dtype=torch.float64, device="cuda"), state=torch.zeros(8, dtype=torch.int32, device="cuda"))
        self.dst = api.PoseGraph(self.ctx, NC, DC, buffers={n: (t[:4] if n == "state" else t[:DC]) for n, t in self.big.items()})
        self.gate = api.ClosureGate(self.ctx, self.src, self.dst, **case["gate"])
        self.poses = torch.full((NC + 2, 12), float(GUARD), dtype=torch.float64, device="cuda")
        self.poses[:NC] = dev(case["poses"])
        self.nd = torch.tensor([case["n"], GUARD, GUARD, GUARD], dtype=torch.int32, device="cuda")
        self.keep = torch.zeros(EC + 8, dtype=torch.uint8, device="cuda")
        self.support = torch.zeros(EC + 8, dtype=torch.int32, device="cuda")
        self.map = torch.zeros(EC + 8, dtype=torch.int32, device="cuda")
        self.info = torch.zeros(8, dtype=torch.int32, device="cuda")
        load_src(self.src, case["log"])

    def run(self):
        EC = self.EC
        for n in ("edge_ij", "edge_Z", "edge_w"):
            self.big[n].fill_(GUARD)
        self.big["state"].fill_(GUARD)
        self.keep.fill_(GUARD8); self.support.fill_(GUARD); self.map.fill_(GUARD); self.info.fill_(GUARD)
        self.gate.run_torch(self.poses[:self.NC], self.nd, keep=self.keep[:EC], support=self.support[:EC], map=self.map[:EC], info=self.info[:4])
        self.ctx.sync()
        assert (host(self.keep)[EC:] == GUARD8).all() and (host(self.support)[EC:] == GUARD).all() and (host(self.map)[EC:] == GUARD).all()
        assert (host(self.info)[4:] == GUARD).all() and (host(self.big["state"])[4:] == GUARD).all()
        return dict(keep=host(self.keep)[:EC].copy(), support=host(self.support)[:EC].copy(), map=host(self.map)[:EC].copy(),
                    info=host(self.info)[:4].copy(), **{n: host(self.big[n]).copy() for n in NAMES})

    def check(self, got, what):
        """byte equality with the restatement; rows >= kept of dst (and the guard row behind the capacity) keep the guard pattern"""
        want, wdst = gn.run_case(self.case, dst_cap=self.DC)
        for n in ("keep", "support", "map", "info"):
            assert same_bytes(got[n], want[n]), (what, n, got[n][:16], want[n][:16])
        kept = int(want["info"][1])
        for n in ("edge_ij", "edge_Z", "edge_w"):
            assert same_bytes(got[n][:kept], getattr(wdst, n)[:kept]), (what, n)
            assert (got[n][kept:] == GUARD).all(), (what, n, "a row >= kept was written")
        assert got["state"][:4].tolist() == wdst.state.tolist(), (what, got["state"])
        return want

    def close(self):
        self.gate.close(); self.dst.close(); self.src.close(); self.ctx.close()


# ------------------------------------------------------------------------------------------------ 1. sizes and counts
@pytest.mark.parametrize("E,cap", [(E, 600) for E in gn.SWEEP_EDGES] + [(32, 32)])
def test_gate_equals_the_restatement_over_edge_counts(E, cap):
    rig = Rig(gn.sweep_case(E, cap=cap), dst_cap=cap + (3 if E == 65 else 0))      # (once with a larger destination)
    want = rig.check(rig.run(), E)
    print(f"   E {E} cap {cap}: valid {want['info'][0]} kept {want['info'][1]} flags {want['info'][3]} largest support {want['support'].max()}")
    assert want["info"][2] == E
    rig.close()


@pytest.mark.parametrize("n", [0, 1, 2])
def test_gate_at_small_node_counts(n):
    rig = Rig(gn.sweep_case(65, n=n))
    want = rig.check(rig.run(), n)
    assert want["info"].tolist() == [0, 0, 65, 0] and (want["support"] == -1).all()    # rows of the second lap are all >= n
    rig.close()


@pytest.mark.parametrize("scribble", [1 << 30, -3])
def test_scribbled_counts_are_clamped_before_they_form_an_address(scribble):
    case = gn.sweep_case(65)
    case["log"].state[0] = scribble                    # the rows behind the 65 edges are zeros: (0, 0) is not valid
    case["n"] = scribble
    rig = Rig(case)
    want = rig.check(rig.run(), scribble)
    assert want["info"][2] == (600 if scribble > 0 else 0) and (want["info"][0] > 0) == (scribble > 0)
    rig.close()


# ------------------------------------------------------------------------------------------------ 2. validity
def test_invalid_edges_have_no_support_and_support_nothing():
    case = gn.validity_case()
    rig = Rig(case)
    got = rig.run()
    rig.check(got, "validity")
    assert (got["support"][case["bad_rows"]] == -1).all() and not got["keep"][case["bad_rows"]].any()
    assert got["info"][0] == len(case["good_rows"]) and got["keep"][case["good_rows"]].all()
    rig.close()


# ------------------------------------------------------------------------------------------------ 3. thresholds in exact arithmetic
@pytest.mark.parametrize("name", sorted(gn.exact_cases()))
def test_thresholds_in_exact_arithmetic(name):
    case, expect = gn.exact_cases()[name]
    rig = Rig(case)
    got = rig.run()
    rig.check(got, name)
    assert got["support"][:len(expect)].tolist() == expect and got["keep"][:len(expect)].tolist() == [int(s >= 1) for s in expect]
    rig.close()


# ------------------------------------------------------------------------------------------------ 4. rounds
@pytest.mark.parametrize("rounds", [1, 2, 3, 8])
def test_the_path_loses_one_edge_from_each_end_a_round(rounds):
    rig = Rig(gn.path_case(rounds))
    got = rig.run()
    rig.check(got, rounds)
    if rounds < 8:
        assert got["keep"][:12].tolist() == [0] * rounds + [1] * (12 - 2 * rounds) + [0] * rounds and got["info"][3] == _lib.GATE_UNSETTLED
    else:
        assert not got["keep"].any() and got["info"].tolist() == [12, 0, 12, 0] and got["state"][:4].tolist() == [0, 0, 0, 0]
    rig.close()


# ------------------------------------------------------------------------------------------------ 5. outliers
def test_the_gate_keeps_the_true_closures_and_the_relaxation_of_them_is_the_clean_graphs():
    case = gn.outlier_case()
    rig = Rig(case)
    got = rig.run()
    rig.check(got, "outlier")
    assert np.flatnonzero(got["keep"]).tolist() == case["true_rows"] and got["info"].tolist() == [11, 8, 11, 0]
    clean = api.PoseGraph(rig.ctx, rig.NC, rig.EC)
    for i, j, Z, w in case["true_edges"]:
        clean.add([i], Z, [1], j, *w)
    for n in ("edge_ij", "edge_Z", "edge_w"):
        assert same_bytes(got[n][:8], host(getattr(clean, n))[:8]), n
    assert same_bytes(got["state"][:4], host(clean.state))
    n = case["n"]
    gated, grep = rig.dst.relax_torch(rig.poses[:n], rig.nd, **case["relax"])
    want, wrep = clean.relax_torch(rig.poses[:n], rig.nd, **case["relax"])
    ungated, urep = rig.src.relax_torch(rig.poses[:n], rig.nd, **case["relax"])
    rig.ctx.sync()
    assert same_bytes(host(gated), host(want)) and same_bytes(host(grep), host(wrep))          # device against device: no tolerance
    gt = case["gt"].reshape(n, 12)
    e_in, e_un, e_ga = (float(np.abs(p - gt).max()) for p in (case["poses"], host(ungated), host(gated)))
    print(f"   outlier case: largest |pose - truth| input {e_in:.3e} ungated relaxation {e_un:.3e} gated relaxation {e_ga:.3e}; "
          f"edges used {host(urep)[-1]:.0f} / {host(grep)[-1]:.0f}")
    assert host(grep)[-1] == n - 1 + 8 and host(urep)[-1] == n - 1 + 11
    assert e_un > e_ga
    clean.close(); rig.close()


# ------------------------------------------------------------------------------------------------ 6. forms
def test_host_form_two_runs_and_null_outputs():
    case = gn.sweep_case(257)
    rig = Rig(case)
    a = rig.run()
    b = rig.run()
    for n in a:
        assert same_bytes(a[n], b[n]), n                # two runs give the same bytes
    rig.check(a, "device form")
    keep, support, mp, info = rig.gate.run(rig.poses[:rig.NC], rig.nd)          # the host form
    assert same_bytes(keep, a["keep"]) and same_bytes(support, a["support"]) and same_bytes(mp, a["map"]) and same_bytes(info, a["info"])
    assert all(same_bytes(host(rig.big[n]), a[n]) for n in NAMES)
    # NULL optional outputs: info and dst as before
    lib, p = rig.ctx.lib, lambda t: C.c_void_p(t.data_ptr())
    for n in ("edge_ij", "edge_Z", "edge_w", "state"):
        rig.big[n].fill_(GUARD)
    rig.info.fill_(GUARD)
    rig.ctx.check(lib.pr_gate_run_dev(rig.gate.h, p(rig.poses), p(rig.nd), None, None, None, p(rig.info)))
    rig.ctx.sync()
    assert same_bytes(host(rig.info)[:4], a["info"]) and (host(rig.info)[4:] == GUARD).all()
    assert all(same_bytes(host(rig.big[n]), a[n]) for n in NAMES)
    hinfo = np.full(4, GUARD, np.int32)
    rig.ctx.check(lib.pr_gate_run(rig.gate.h, p(rig.poses), p(rig.nd), None, None, None, hinfo.ctypes.data_as(C.c_void_p)))
    assert same_bytes(hinfo, a["info"])
    err = lambda: lib.pr_last_error(rig.ctx.h)
    for who in range(3):                               # d_poses, d_n, d_info are required
        args = [p(rig.poses), p(rig.nd), p(rig.info)]
        args[who] = None
        assert lib.pr_gate_run_dev(rig.gate.h, args[0], args[1], None, None, None, args[2]) == _lib.PR_EINVAL and b"a required pointer is NULL" in err()
        assert lib.pr_gate_run(rig.gate.h, args[0], args[1], None, None, None, args[2]) == _lib.PR_EINVAL and b"a required pointer is NULL" in err()
    with pytest.raises(ValueError, match="support must be"):
        rig.gate.run_torch(rig.poses[:rig.NC], rig.nd, support=torch.zeros(rig.EC, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="keep must be"):
        rig.gate.run_torch(rig.poses[:rig.NC], rig.nd, keep=torch.zeros(rig.EC + 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="info must be"):
        rig.gate.run_torch(rig.poses[:rig.NC], rig.nd, info=torch.zeros(4, dtype=torch.int32))
    rig.close()


def test_one_capture_of_gate_and_relax_on_the_empty_log_serves_every_count():
    case = gn.outlier_case()
    edges = [(int(i), int(j), Z, w) for (i, j), Z, w in zip(case["log"].edge_ij[:11], case["log"].edge_Z[:11], case["log"].edge_w[:11])]
    prm = dict(case["relax"], outer=3, inner=60)
    N, EC = 44, 16
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        src = api.PoseGraph(ctx, N, EC, max_outer=3, max_inner=60)
        dst = api.PoseGraph(ctx, N, EC, max_outer=3, max_inner=60)
        gate = api.ClosureGate(ctx, src, dst, **case["gate"])
        poses = torch.zeros((N, 12), dtype=torch.float64, device="cuda")
        poses[:40] = dev(case["poses"])
        nd = torch.zeros(4, dtype=torch.int32, device="cuda")               # a map's state: word 0 is the count - 0 at the capture
        outs = dict(keep=torch.zeros(EC, dtype=torch.uint8, device="cuda"), support=torch.zeros(EC, dtype=torch.int32, device="cuda"),
                    map=torch.zeros(EC, dtype=torch.int32, device="cuda"), info=torch.zeros(4, dtype=torch.int32, device="cuda"))
        out = torch.zeros((N, 12), dtype=torch.float64, device="cuda")
        rep = torch.zeros(5, dtype=torch.float64, device="cuda")
        gate.run_torch(poses, nd, **outs)                                    # one eager call, then the capture of the same calls
        dst.relax_torch(poses, nd, out=out, report=rep, **prm)
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            gate.run_torch(poses, nd, **outs)
            dst.relax_torch(poses, nd, out=out, report=rep, **prm)
        model = pg.PoseGraphModel(EC)
        kept_seen, moved = [], 0
        for n, count in ((12, 4), (33, 8), (40, 11)):                        # three node and edge counts under the one capture
            while src.count()[0] < count:
                i, j, Z, w = edges[src.count()[0]]
                src.add([i], Z, [1], j, *w); model.add([i], Z, [1], j, *w)
            nd[0] = n
            for t in outs.values():
                t.fill_(GUARD8 if t.dtype == torch.uint8 else GUARD)
            out.fill_(GUARD); rep.fill_(GUARD)
            graph.replay()
            st.synchronize()
            a = {k: host(t).copy() for k, t in outs.items()}
            a_out, a_rep, a_dst = host(out).copy(), host(rep).copy(), {nm: host(getattr(dst, nm)).copy() for nm in NAMES}
            e = gate.run_torch(poses, nd)                                    # eager, fresh buffers
            o2, r2 = dst.relax_torch(poses, nd, **prm)
            st.synchronize()
            for k, t in zip(("keep", "support", "map", "info"), e):
                assert same_bytes(a[k], host(t)), (n, count, k)
            assert same_bytes(a_out[:n], host(o2)[:n]) and same_bytes(a_rep, host(r2)) and (a_out[n:] == GUARD).all(), (n, count)
            assert all(same_bytes(a_dst[nm], host(getattr(dst, nm))) for nm in NAMES)
            want = gn.gate(host(poses), n, model, N, **case["gate"])
            for k in ("keep", "support", "map", "info"):
                assert same_bytes(a[k], want[k]), (n, count, k, a[k], want[k])
            kept_seen.append(int(a["info"][1]))
            moved += int(not same_bytes(a_out[:n], host(poses)[:n]))
        assert kept_seen[0] == 0 and kept_seen[2] == 8 and moved >= 2, (kept_seen, moved)
        del graph
        gate.close(); dst.close(); src.close(); ctx.close()


def test_the_source_logs_overflow_is_mirrored():
    case = gn.outlier_case()
    ctx = _stream_context(0)
    src, dst = api.PoseGraph(ctx, 40, 6), api.PoseGraph(ctx, 40, 6)
    model, wdst = pg.PoseGraphModel(6), pg.PoseGraphModel(6)
    for i, j, Z, w in case["true_edges"]:              # eight adds into six rows
        src.add([i], Z, [1], j, *w); model.add([i], Z, [1], j, *w)
    assert src.count() == (6, _lib.POSEGRAPH_OVERFLOW)
    gate = api.ClosureGate(ctx, src, dst, **case["gate"])
    nd = torch.tensor([40], dtype=torch.int32, device="cuda")
    keep, support, mp, info = gate.run_torch(dev(case["poses"]), nd)
    ctx.sync()
    want = gn.gate(case["poses"], 40, model, 40, dst=wdst, **case["gate"])
    assert same_bytes(host(info), want["info"]) and host(info).tolist() == [6, 6, 6, _lib.GATE_SRC_OVERFLOW]
    assert same_bytes(host(keep), want["keep"]) and same_bytes(host(support), want["support"]) and same_bytes(host(mp), want["map"])
    assert host(dst.state).tolist() == [6, _lib.POSEGRAPH_OVERFLOW, 0, 0] == wdst.state.tolist()
    for nm in ("edge_ij", "edge_Z", "edge_w"):
        assert same_bytes(host(getattr(dst, nm)), getattr(wdst, nm)), nm
    gate.close(); dst.close(); src.close(); ctx.close()
