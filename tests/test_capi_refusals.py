"""Every refusal of the fourteen header-block decoder entry points (include/hhuff.h hhuff_hpack_{decode_blocks,
parse_requests,parse_responses} and hhuff_qpack_{decode,parse_requests,parse_responses}, their _slots twins and the
two _sessions calls): the return code and the whole hhuff_last_error_string().  No call here reaches the device:
each is refused by an argument check, or returns at nconn == 0.  Pointers are dummy aligned addresses that are
never dereferenced.  The messages are written out here, check by check, in the order include/hhuff.h's entry
points make them."""
import ctypes

import pytest

from h2o_amd import codec

P = 1 << 20  # a 256-byte aligned dummy address
T = 4096     # table size of the good calls
NCONN = 2

HPACK_TAIL = ["scratch", "scratch_size", "flags", "stream"]
HPACK_HEAD = ["in", "in_size", "blk_off", "conn_first", "nconn", "table_size"]
HPACK_OUT = ["arena", "arena_off", "name_off", "name_len", "value_off", "value_len", "fflags", "nfields", "bstatus"]
QPACK_HEAD = ["in", "in_size", "enc_off", "enc_len", "sec_off", "conn_first", "nconn", "nsec", "table_size",
              "max_blocked", "num_blocked"]
QPACK_SEC = ["arena", "arena_off", "name_off", "name_len", "value_off", "value_len", "fflags", "nfields", "sstatus",
             "req_insert_count"]
QPACK_ENC = ["enc_status", "enc_consumed", "insert_count"]

# entry point -> its arguments behind the optional (ds, slots), in the public order
ORDER = {
    "hhuff_hpack_decode_blocks": HPACK_HEAD + HPACK_OUT + HPACK_TAIL,
    "hhuff_hpack_parse_requests": HPACK_HEAD + HPACK_OUT + ["req"] + HPACK_TAIL,
    "hhuff_hpack_parse_responses": HPACK_HEAD + ["trailers"] + HPACK_OUT + ["res"] + HPACK_TAIL,
    "hhuff_qpack_decode": QPACK_HEAD + QPACK_SEC + QPACK_ENC + HPACK_TAIL,
    "hhuff_qpack_parse_requests": QPACK_HEAD + QPACK_SEC + QPACK_ENC + ["stream_id", "req"] + HPACK_TAIL,
    "hhuff_qpack_parse_responses": QPACK_HEAD + QPACK_SEC + QPACK_ENC + ["stream_id", "res"] + HPACK_TAIL,
}
HPACK = [n for n in ORDER if "hpack" in n]
QPACK = [n for n in ORDER if "qpack" in n]
SESSIONS = ["hhuff_qpack_parse_requests_sessions", "hhuff_qpack_parse_responses_sessions"]
ENTRY_POINTS = HPACK + [n + "_slots" for n in HPACK] + QPACK + [n + "_slots" for n in QPACK] + SESSIONS
assert len(ENTRY_POINTS) == 14

SCALARS = {"in_size": 100, "nconn": NCONN, "table_size": T, "nsec": 3, "max_blocked": 16, "flags": 0}
DS_MEMBERS = ["state", "cancel_first", "cancel_id", "cancel_flags", "dec_out", "dec_out_off", "dec_out_len", "wake_id",
              "wake_first", "nwake", "parked", "dflags"]


def base_of(name):
    for suffix in ("_slots", "_sessions"):
        if name.endswith(suffix):
            return name[:-len(suffix)]
    return name


def has_slots(name):
    return name.endswith("_slots") or name.endswith("_sessions")


class Refusals:
    def __init__(self):
        self.L = codec.lib()

    def scratch_size(self, name, nconn=NCONN, table_size=T):
        f = self.L.hhuff_hpack_scratch_size if "hpack" in name else self.L.hhuff_qpack_scratch_size
        return int(f(nconn, table_size))

    def call(self, name, slots=None, ds=None, **over):
        """the entry point with good arguments, `over` replacing some; slots: None, or (slot, flags, nslots);
        ds: for the session calls a dict of member overrides, or "null" """
        order = list(ORDER[base_of(name)])
        if name.endswith("_sessions"):
            order.remove("num_blocked")
        args = {}
        for a in order:
            args[a] = SCALARS.get(a, P)
        args["stream"] = None
        args["num_blocked"] = None
        args["trailers"] = None
        args["scratch_size"] = self.scratch_size(name, over.get("nconn", NCONN), over.get("table_size", T))
        args.update(over)
        head = []
        keep = []
        if name.endswith("_sessions"):
            if ds == "null":
                head.append(None)
            else:
                mb = min(args["max_blocked"], 4096)
                nstate = slots[2] if slots else args["nconn"]
                members = dict({m: P for m in DS_MEMBERS}, flags=0,
                               state_size=int(self.L.hhuff_qpack_dsession_state_size(nstate, mb)))
                members.update(ds or {})
                s = codec._QpackDsessionsStruct(**members)
                keep.append(s)
                head.append(ctypes.byref(s))
        if has_slots(name):
            if slots is None:
                head.append(None)
            else:
                s = codec._ConnSlotsStruct(slot=slots[0], flags=slots[1], nslots=slots[2])
                keep.append(s)
                head.append(ctypes.byref(s))
        rc = getattr(self.L, name)(*(head + [args[a] for a in order]))
        return rc, self.L.hhuff_last_error_string().decode()


@pytest.fixture(scope="module")
def R():
    return Refusals()


def refused(R, why, name, **kw):
    rc, err = R.call(name, **kw)
    assert rc == -1 and err == "invalid argument: " + why, (name, kw, rc, err)


def required_arrays(name):
    """the arrays hpack_blocks / qpack_step refuse as NULL (QPACK: nsec != 0 in the good call)"""
    if "hpack" in name:
        return ["in", "blk_off", "conn_first"] + HPACK_OUT + ["scratch"]
    return ["in", "enc_off", "enc_len", "sec_off", "conn_first"] + QPACK_ENC + ["scratch"] + QPACK_SEC


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_nconn_zero_returns_ok(R, name):
    """nothing to do: HHUFF_OK whatever the arrays are (the entry point's own alignment checks still hold)"""
    over = {a: None for a in required_arrays(name)}
    assert R.call(name, nconn=0, scratch_size=0, **over)[0] == 0
    if has_slots(name):
        assert R.call(name, slots=(None, None, 4), nconn=0, scratch_size=R.scratch_size(name, 4), **over)[0] == 0


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_null_arrays(R, name):
    for a in required_arrays(name):
        refused(R, "NULL array", name, **{a: None})
    own = [a for a in ("req", "res") if a in ORDER[base_of(name)]]
    if "qpack" in name and own:
        own.append("stream_id")
    for a in own:  # the entry point's own pre-check
        refused(R, "NULL array", name, **{a: None})
    if "qpack" in name:  # without sections the section arrays (and stream_id, req, res) may be NULL ...
        over = {a: None for a in QPACK_SEC + own}
        # ... and the call gets as far as the next refusal
        refused(R, "scratch must be 16-byte aligned", name, nsec=0, scratch=P + 8, **over)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_scratch(R, name):
    ss = R.scratch_size(name)
    which = "hhuff_hpack_scratch_size" if "hpack" in name else "hhuff_qpack_scratch_size"
    refused(R, "scratch smaller than " + which, name, scratch_size=ss - 1)
    refused(R, "scratch must be 16-byte aligned", name, scratch=P + 8)
    if has_slots(name):
        slab = ss // NCONN
        refused(R, "scratch smaller than nslots slabs", name, slots=(None, None, 5), scratch_size=5 * slab - 1)
        refused(R, "scratch must be 16-byte aligned", name, slots=(None, None, 5), scratch_size=5 * slab, scratch=P + 8)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_record_alignment(R, name):
    order = ORDER[base_of(name)]
    if "req" in order:
        refused(R, "req must be 8-byte aligned", name, req=P + 4)
    if "res" in order:
        if "hpack" in name:
            refused(R, "res must be 4-byte aligned", name, res=P + 2)
        else:
            refused(R, "res must be 8-byte aligned", name, res=P + 4)
    if "qpack" in name and ("req" in order or "res" in order):  # checked before nconn == 0
        a = "req" if "req" in order else "res"
        refused(R, a + " must be 8-byte aligned", name, nconn=0, **{a: P + 4})


@pytest.mark.parametrize("name", [n for n in ENTRY_POINTS if has_slots(n)])
def test_bad_conn_slots(R, name):
    big = 1 << 62
    refused(R, "slots: nslots is 0", name, slots=(None, None, 0), scratch_size=big)
    refused(R, "slots: nslots above 2^31 - 1", name, slots=(None, None, 1 << 31), scratch_size=big)
    refused(R, "slots: nconn above nslots without a slot array", name, slots=(None, None, 1), scratch_size=big)
    refused(R, "slots: nconn above nslots without a slot array", name, slots=(None, P, 1), scratch_size=big)
    # refused even when there is nothing to do
    refused(R, "slots: nslots is 0", name, slots=(None, None, 0), scratch_size=big, nconn=0)


@pytest.mark.parametrize("name", [n for n in ENTRY_POINTS if "qpack" in n])
def test_qpack_sizes(R, name):
    why = "in_size must be at most 2^32 - 3 (u32 offsets)"
    refused(R, why, name, in_size=(1 << 32) - 2)
    refused(R, why, name, in_size=1 << 32)
    refused(R, "header_table_size above 2^30", name, table_size=(1 << 30) + 1)
    if has_slots(name):  # with slots: in front of the slot checks
        refused(R, "header_table_size above 2^30", name, table_size=(1 << 30) + 1, slots=(None, None, 0))
        refused(R, why, name, in_size=(1 << 32) - 2, slots=(None, None, 5), scratch_size=1 << 62)


@pytest.mark.parametrize("name", SESSIONS)
def test_sessions(R, name):
    refused(R, "sessions: NULL hhuff_qpack_dsessions_t", name, ds="null")
    assert R.call(name, ds="null", nconn=0)[0] == 0
    refused(R, "sessions: max_blocked above 4096", name, max_blocked=4097)
    refused(R, "sessions: max_blocked above 4096", name, max_blocked=4097, nconn=0)
    refused(R, "sessions: max_blocked above 4096", name, max_blocked=4097, ds="null", slots=(None, None, 0))
    refused(R, "sessions: nconn above 2^31 - 1", name, nconn=1 << 31, scratch_size=0)
    refused(R, "sessions: nconn above 2^31 - 1", name, nconn=1 << 31, slots=(P, None, 1))
    for m in DS_MEMBERS:
        if m in ("cancel_first", "cancel_id", "cancel_flags"):
            continue
        refused(R, "sessions: NULL array", name, ds={m: None})
    refused(R, "sessions: NULL array", name, ds={"cancel_id": None})  # cancel_first without cancel_id
    # in front of the call's own arrays
    refused(R, "sessions: NULL array", name, ds={"state": None}, **{"in": None})
    # optional members: the call goes on to the next refusal
    refused(R, "scratch must be 16-byte aligned", name, scratch=P + 8,
            ds={"cancel_first": None, "cancel_id": None, "cancel_flags": None})
    refused(R, "scratch must be 16-byte aligned", name, scratch=P + 8, max_blocked=0, ds={"wake_id": None})
    refused(R, "sessions: unknown flag bit", name, ds={"flags": 2})
    refused(R, "sessions: unknown flag bit", name, ds={"flags": 1 | 1 << 31})
    refused(R, "scratch must be 16-byte aligned", name, scratch=P + 8, ds={"flags": 1})
    size = int(R.L.hhuff_qpack_dsession_state_size(NCONN, 16))
    why = "sessions: state smaller than hhuff_qpack_dsession_state_size"
    refused(R, why, name, ds={"state_size": size - 1})
    slot_size = int(R.L.hhuff_qpack_dsession_state_size(5, 16))  # with slots: one session per slot
    slab = R.scratch_size(name) // NCONN
    refused(R, why, name, slots=(None, None, 5), scratch_size=5 * slab, ds={"state_size": slot_size - 1})
    refused(R, "sessions: state must be 16-byte aligned", name, ds={"state": P + 8})
    refused(R, "NULL array", name, **{"in": None})  # behind the session checks
