"""The HTTP/2 scheduler on the device (include/hhuff.h (2o)): hhuff_h2_schedule through codec.h2_schedule against
tests/golden/h2sched.npz, what h2o's own lib/http2/scheduler.c did with the same ops and runs (tools/gen_h2sched_fixture.py).
A case is a connection and a step is a call, so the cases of a test run side by side through connection slots, begin at
different calls (HHUFF_CONN_RESET beside continuing connections) and drop out as they end (sparse slot lists).  Equality
throughout: the visit order, the statuses, the root's activity and every stream's parent and weight after each call."""
import numpy as np
import pytest

import bounds_harness as B
from conftest import load_golden

pytestmark = pytest.mark.gpu
MN = 131  # the largest tree of the fixture, and one more


@pytest.fixture(scope="module")
def G():
    g = dict(load_golden("h2sched"))
    g["names"] = g["names"].tobytes().decode().split("\n")
    return g


def _tensor(torch, a):
    """the records' bytes on the device (never an empty tensor: the call wants an address)"""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([raw, np.zeros(max(0, 32 - raw.size), np.uint8)])).cuda()


def _first(torch, counts):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32).view(np.int32)).cuda()


def _inputs(torch, C, G, steps):
    """the arrays of one call whose connections are the fixture's steps `steps`"""
    ops = np.zeros(0, C.H2_SCHED_OP_DTYPE)
    sends = np.zeros(0, C.H2_SEND_DTYPE)
    peers = C.h2_new_peers(len(steps))
    nop, ncand, room = [], [], []
    for c, s in enumerate(steps):
        o = G["ops"][G["op_first"][s]:G["op_first"][s + 1]]
        rec = np.zeros(len(o), C.H2_SCHED_OP_DTYPE)
        for k, f in enumerate(("stream_id", "op", "parent_id", "weight", "exclusive")):
            rec[f] = o[:, k]
        ops = np.concatenate([ops, rec])
        d = G["cands"][G["cand_first"][s]:G["cand_first"][s + 1]]
        rec = np.zeros(len(d), C.H2_SEND_DTYPE)
        rec["stream_id"], rec["body_len"], rec["window"], rec["flags"] = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
        sends = np.concatenate([sends, rec])
        peers[c]["send_window"], peers[c]["max_frame_size"] = G["conn"][s][0], G["conn"][s][2]
        nop.append(len(o)), ncand.append(len(d)), room.append(int(G["conn"][s][1]))
    return dict(ops=_tensor(torch, ops) if len(ops) else None, op_first=_first(torch, nop), sends=_tensor(torch, sends),
                send_first=_first(torch, ncand), nsend=len(sends), nop=len(ops), peers=_tensor(torch, peers), out_off=_first(torch, room), out_size=sum(room))


def _play(G, cases, max_nodes=MN, nslots=None, stagger=3, each=None):
    """run the named cases side by side, connection j from call j % stagger on, in slot nslots - 1 - 2j of a scratch of
    nslots slots; every call is compared with the fixture.  each(step list, inputs, result): a further check a call."""
    import torch

    from h2o_amd import codec as C

    conns = [G["names"].index(x) for x in cases]  # connection j plays case conns[j]
    nslots = nslots or 2 * len(conns)
    scratch = torch.full((C.h2_sched_scratch_size(nslots, max_nodes),), 0xA5, dtype=torch.uint8, device="cuda")
    nstep = [int(G["case_first"][k + 1] - G["case_first"][k]) for k in conns]
    for call in range(max(j % stagger + n for j, n in enumerate(nstep))):
        live = [j for j, n in enumerate(nstep) if 0 <= call - j % stagger < n]
        steps = [int(G["case_first"][conns[j]]) + call - j % stagger for j in live]
        I = _inputs(torch, C, G, steps)
        slots = C.ConnSlots(torch.tensor([nslots - 1 - 2 * j for j in live], dtype=torch.int32, device="cuda"),
                            torch.tensor([C.CONN_RESET if call == j % stagger else 0 for j in live], dtype=torch.uint8, device="cuda"), nslots)
        r = C.h2_schedule(max_nodes, scratch, I["sends"], I["send_first"], I["peers"], I["out_off"], ops=I["ops"], op_first=I["op_first"],
                          flags=C.H2SC_CONTINUE, slots=slots, nsend=I["nsend"], out_size=I["out_size"])
        ordered = r["ordered"].cpu().numpy()[:24 * I["nsend"]].view(C.H2_SEND_DTYPE)
        nvisit, first, active, host = r["nvisit"].cpu().numpy(), I["send_first"].cpu().numpy(), r["active"].cpu().numpy(), scratch.cpu()
        assert not r["cstatus"].cpu().numpy().any() and (I["ops"] is None or not r["op_status"].cpu().numpy()[:I["nop"]].any())
        for c, (j, s) in enumerate(zip(live, steps)):
            what = "%s step %d" % (G["names"][conns[j]], s - G["case_first"][conns[j]])
            want = G["visits"][G["visit_first"][s]:G["visit_first"][s + 1]]
            assert ordered["stream_id"][first[c]:first[c] + nvisit[c]].tolist() == want[:, 0].tolist(), what
            assert active[c] == G["active"][s], what
            tree = {int(i): (int(p), int(w)) for i, p, w in G["tree"][G["tree_first"][s]:G["tree_first"][s + 1]]}
            assert C.h2_sched_tree(host, nslots - 1 - 2 * j, max_nodes) == tree, what
        if each:
            each(steps, I, r)


TREE_EDITS = (["excl_open_0", "excl_open_1", "excl_open_3", "rebind_no_change", "parent_missing", "w257", "rebind_grandchild",
               "unit_reprioritize_0", "unit_reprioritize_1", "rebind_child_0", "rebind_child_1", "unit_exclusive_at_pos", "unit_exclusive", "chain_16"] +
              ["close_%d_%s" % (p, w) for p in (1, 16, 257) for w in ("1_256", "16_16_16", "256_256", "257")])
QUEUES = ["queue_1_16", "queue_1_16_256", "queue_16_256_256", "queue_1_16_credit", "queue_1_16_256_credit", "queue_16_256_256_credit",
          "inactive_parent", "deactivate_queued", "unit_queue", "unit_round_robin", "unit_priority", "unit_dependency", "unit_firefox",
          "unit_change_weight"]
RUNS = ["bail_conn_window", "bail_room", "entry_window_0", "partial_frames"]


@pytest.mark.parametrize("cases", [TREE_EDITS, QUEUES, RUNS, ["flat_1", "flat_63", "flat_64", "flat_65", "flat_130"], ["unit_firefox"],
                                   ["w257", "bail_room"]], ids=["tree_edits", "queues", "runs", "lane_edges", "batch_1", "batch_2"])
def test_visits_and_trees_equal_h2o(G, cases):
    _play(G, cases)


def test_table_at_max_nodes_and_65_connections(G):
    """tables with no entry to spare, five entries a lane, and the interface's limit; 65 connections a call"""
    _play(G, ["flat_130"], max_nodes=130, stagger=1)
    _play(G, ["flat_300"], max_nodes=301, stagger=1)
    _play(G, ["chain_16", "flat_300"], max_nodes=2048, nslots=5)
    _play(G, ["bail_room", "unit_exclusive", "close_16_16_16_16", "partial_frames", "excl_open_3"] * 13, nslots=129)


def test_closed_loop_with_the_framer(G):
    """the ordered records given to hhuff_h2_frame_data send what the fixture's callback sent, visit by visit"""
    import torch

    from h2o_amd import codec as C

    body = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")

    def each(steps, I, r):
        f = C.h2_frame_data(body, r["ordered"], I["send_first"], I["peers"], I["out_off"], nsend=I["nsend"], out_size=I["out_size"])
        sent, first = f["sent"].cpu().numpy()[:24 * I["nsend"]].view(C.H2_SENT_DTYPE)["sent"], I["send_first"].cpu().numpy()
        assert not f["cstatus"].cpu().numpy().any()
        for c, s in enumerate(steps):
            want = G["visits"][G["visit_first"][s]:G["visit_first"][s + 1], 1].tolist()
            assert sent[first[c]:first[c + 1]].tolist() == want + [0] * (first[c + 1] - first[c] - len(want)), s

    _play(G, RUNS + ["unit_dependency", "w257"], each=each)


def test_hostile_ops_and_ranges_stay_inside():
    """malformed ops, ranges beyond the arrays, a candidate of an unknown stream, a duplicate stream, a refused slot: the
    statuses of (2o), every record still listed once, and no byte outside the arrays' declared sizes"""
    import torch

    from h2o_amd import codec as C

    O, R, X, A = C.H2Q_OPEN, C.H2Q_REBIND, C.H2Q_CLOSE, C.H2Q_ACTIVATE
    ops = np.array([(1, O, 0, 16, 0, 0), (1, O, 0, 16, 0, 0), (3, O, 1, 257, 1, 0), (5, O, 0, 1, 0, 0), (7, A, 0, 0, 0, 0), (3, R, 3, 16, 0, 0),
                    (0, O, 0, 16, 0, 0), (3, 9, 0, 0, 0, 0), (3, O, 0, 258, 0, 0), (3, X, 1, 0, 0, 0), (3, A, 0, 0, 0, 1), (3, R, 0, 0, 2, 0),
                    (3, A, 0, 0, 0, 0), (1, A, 0, 0, 0, 0), (1, O, 0, 16, 0, 0)], C.H2_SCHED_OP_DTYPE)
    want = [0, C.H2SC_EEXIST, 0, C.H2SC_EFULL, C.H2SC_ENOENT] + [C.H2SC_EINVAL] * 7 + [0, 0] + [C.H2SC_ESLOT]
    sends = np.zeros(5, C.H2_SEND_DTYPE)
    sends["stream_id"], sends["body_len"], sends["window"], sends["flags"] = [9, 1, 1, 0, 3], 5, [9, 9, 9, 9, 9], [1, 4, 1, 0xFFFFFFFF, 1]
    fill = 0x5A
    bufs = {k: B.guarded(torch, n, fill) for k, n in (("ordered", 24 * 5), ("order", 4 * 5), ("pos", 4 * 5), ("op_status", 4 * 15),
                                                      ("nvisit", 4 * 3), ("cstatus", 4 * 3), ("active", 3), ("scratch", C.h2_sched_scratch_size(2, 2)))}
    out = {k: (v[1] if k in ("ordered", "active") else v[1].view(torch.int32)) for k, v in bufs.items() if k != "scratch"}
    i32 = lambda a: torch.tensor(np.array(a, np.uint32).view(np.int32), device="cuda")  # noqa: E731
    slots = C.ConnSlots(i32([1, 7, 1]), None, 2)  # connection 1: no such slot; connection 2: slot 1 is taken
    r = C.h2_schedule(2, bufs["scratch"][1], _tensor(torch, sends), i32([0, 5, 0xFFFFFFF0, 0xFFFFFFFF]), _tensor(torch, C.h2_new_peers(3)),
                      i32([0, 4096, 0xFFFFFFFF, 7]), ops=_tensor(torch, ops), op_first=i32([0, 14, 14, 0xFFFFFFFF]), slots=slots, out_size=4096, out=out)
    torch.cuda.synchronize()
    assert r["op_status"].cpu().tolist() == want
    assert r["cstatus"].cpu().tolist() == [0, C.H2SC_ESLOT, C.H2SC_ESLOT] and r["nvisit"].cpu().tolist() == [2, 0, 0]
    ordered = r["ordered"].cpu().numpy().view(C.H2_SEND_DTYPE)
    assert ordered["stream_id"].tolist() == [1, 3, 9, 1, 0] and ordered["window"].tolist() == [9, 9, 0, 0, 0]
    assert r["order"].cpu().tolist() == [2, 4, 0, 1, 3] and r["pos"].cpu().tolist() == [2, 3, 0, 4, 1]  # record 1: an unknown flag
    assert C.h2_sched_tree(bufs["scratch"][1], 1, 2) == {1: (0, 16), 3: (1, 257)} and r["active"].cpu().tolist() == [0, 0, 0]
    for k, (whole, inner) in bufs.items():
        guards = torch.cat([whole[:B.GUARD], whole[whole.numel() - B.GUARD:]])
        assert bool((guards == fill).all()), k
    assert bool((bufs["scratch"][1][:C.h2_sched_scratch_size(1, 2)] == fill).all())  # slot 0 belongs to no connection
