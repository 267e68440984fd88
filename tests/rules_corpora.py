"""The hand-built corpus of h2o's request / response rules (lib/http2/hpack.c:502-750) and the routes by which a
field's name class and value bytes reach them in the kernels -- plain helpers, no GPU.

A case is a field list, the parsers it is for (rules_model.PARSERS) and its LITERAL expected result, written in the
case in HTTP/2 terms: E(verdict, header flags, record fields).  expect_for() adds only what lib/http3/qpack.c adds
for the h3 parsers (a hard verdict becomes DECOMPRESSION_FAILED, a refused name has decode_header's own
description).  The model (rules_model.py) has to agree with these; they are not derived from it.

The DECISIVE field of a case (the last one unless `at` says otherwise) is the one whose name class or value bytes
decide the outcome.  hpack_variants() / qpack_variants() put it on the wire by every route that applies:

  HPACK   lit_raw / lit_huff       a literal name and value, raw / Huffman (req_name_class on kSrcIn / kSrcLit bytes)
          static_idx / static_ref  a static index (s_scls[], kSrcStatic) / a literal value with a static name index
          same_idx / same_ref      a dynamic index / name index whose entry an earlier block of THIS call inserted
                                   in the same mode (Entry::cls cached; the value still at kSrcIn)
          earlier_idx / _ref       the same, the entry inserted by an EARLIER call in the same mode (value in the ring)
          plain_idx / plain_ref    the entry inserted by a plain-mode call (kClsUnknown, recomputed per reference)
          (an entry that arrived through hhuff_conn_import: test_rule_edges.py moves the plain_* scratch)
  QPACK   lit_raw / lit_huff, static_idx / static_ref, dyn_idx / dyn_ref, post_idx / post_ref

Where a case names a `follow` byte (what the rule would accept next: the `s` behind `trailer`, a digit behind 18
digits, the `0` behind `20`), the decisive field ends its block and that byte comes next: as the first byte of the
next connection's block in the input, and as the names and values of the entries inserted around the decisive one in
the rings.  A read past the value's length then changes the answer.  (Behind a Huffman literal's decoded bytes lies
the rest of its floor(8 len / 5) slot, which no input byte controls.)

Routes that cannot be reached are returned by hpack_variants() / qpack_variants() as (case, route, why) beside the
variants, not dropped silently:
  - an entry can be inserted in the same mode only by a block that survives it: a value (or name) that is a hard
    error in that mode kills the connection at the insert, so same_idx / earlier_idx exist only for decisive fields
    that are accepted where they are inserted, and same_ref / earlier_ref only for names with an acceptable value;
  - static_idx needs the exact (name, value) pair in the static table: the only bad content-length a static index
    can carry is the empty one (HPACK 28), the only te none;
  - a field with soft-error bits keeps them only as the literal it arrived as; an upper-case name never enters a
    table."""
import functools

from blocks_harness import (ccase, indexed, literal, q_indexed, q_indexed_post, q_insert, q_literal, q_literal_post,
                            q_literal_ref, q_prefix, qcase, qstr, string)
from bounds_harness import huffman
from h2o_amd import tables
from rules_model import DECOMPRESSION_FAILED, E_DECODE, E_UPPER, NO_LENGTH, SOFT, UPPER

HSTATIC, QSTATIC = tables.STATIC_TABLE, tables.QPACK_STATIC_TABLE  # HPACK index i = HSTATIC[i - 1]
H2_REQ, H3_REQ, REQ = ("h2_req",), ("h3_req",), ("h2_req", "h3_req")
H2_RES, H3_RES, HEAD, TRAILERS = ("h2_res",), ("h3_res",), ("h2_res", "h3_res"), ("h2_trailers",)
RES = HEAD + TRAILERS
REQ_DEFAULTS = dict(content_length=NO_LENGTH, method=-1, scheme=-1, authority=-1, path=-1, protocol=-1, expect=-1,
                    exists_map=0, err=0, scheme_kind=0, datagram_flow_id=-1)
RES_DEFAULTS = dict(status=0, err=0, datagram_flow_id=-1)


def E(verdict, header, **rec):
    """a literal expectation: the verdict in HTTP/2 terms, one '1' / '0' per decoded field (listed or not), and the
    record fields that differ from a reset record (nheaders is the number of '1's)"""
    return dict(verdict=verdict, header=header, rec=rec)


def expect_for(case, parser):
    """-> dict(verdict, nfields, header=[0/1], rec): the case's expectation for one of its parsers"""
    e = case["expect"]
    defaults = REQ_DEFAULTS if parser.endswith("req") else RES_DEFAULTS
    assert set(e["rec"]) <= set(defaults), case["name"]
    rec = dict(defaults, **e["rec"])
    rec["nheaders"] = e["header"].count("1")
    verdict = e["verdict"]
    if parser.startswith("h3"):
        if verdict not in (0, SOFT):
            verdict = DECOMPRESSION_FAILED
        if rec["err"] == E_UPPER:
            rec["err"] = E_DECODE
    return dict(verdict=verdict, nfields=len(e["header"]), header=[int(c) for c in e["header"]], rec=rec)


def record_words(rec, parser):
    """the record as the u32 words of hhuff_request_t (+ datagram_flow_id for h3) / hhuff_response_t"""
    u = lambda v: v & 0xFFFFFFFF  # noqa: E731
    if parser.endswith("req"):
        w = [u(rec["content_length"]), rec["content_length"] >> 32] + [u(rec[k]) for k in (
            "method", "scheme", "authority", "path", "protocol", "expect", "exists_map", "nheaders", "err", "scheme_kind")]
        return w + [u(rec["datagram_flow_id"])] if parser == "h3_req" else w
    return [u(rec[k]) for k in ("status", "nheaders", "err", "datagram_flow_id")]


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
GET, HTTPS, ROOT = (b":method", b"GET", 0), (b":scheme", b"https", 0), (b":path", b"/", 0)
P3 = [GET, HTTPS, ROOT]  # fields 0, 1, 2 of most request cases
OK3 = dict(method=0, scheme=1, path=2, exists_map=7, scheme_kind=2)
S200 = (b":status", b"200", 0)
DATE = (b"date", b"", 0)  # a one-byte indexed field in both static tables (HPACK 33, QPACK 6)


Q_RAW_ROUTES = ("lit_raw", "dyn_idx", "post_idx", "dyn_ref", "post_ref")


def F(name, value=b"", soft=0):
    return (name, value, soft)


def _cases():
    out = []

    def C(name, parsers, fields, expect, follow=None, at=None, routes=None):
        out.append(dict(name=name, parsers=parsers, fields=list(fields), expect=expect, follow=follow,
                        at=len(fields) - 1 if at is None else at, routes=routes))

    def Cp(name, h2, h3, fields, expect, expect_raw=None):
        """a case whose decisive name starts with a colon and is no token.  HPACK hands such a name over unvalidated
        (hpack.c:141, :249), and so does a Huffman literal in QPACK; QPACK's raw literal looks the token up and
        validates the rest (qpack.c:583-587, :375 on the encoder stream), where the colon is an invalid character (a
        soft name error) and an upper-case letter a hard one.  fields(soft) -> the field list"""
        C(name, h2, fields(0), expect)
        C(name + ", raw in QPACK", h3, fields(1), expect_raw or expect, routes=Q_RAW_ROUTES)
        C(name + ", Huffman in QPACK", h3, fields(0), expect, routes=("lit_huff",))

    CL = b"content-length"
    # ---- content-length (hpack.c:592-597, h2o_strtosize) ------------------------------------------
    C("content-length empty", REQ, P3 + [F(CL, b"")], E(-1, "0000", err=5, **OK3))  # HPACK static 28 as it is
    C("content-length 0", REQ, P3 + [F(CL, b"0")], E(0, "0000", content_length=0, **OK3))
    C("content-length 7", REQ, P3 + [F(CL, b"7")], E(0, "0000", content_length=7, **OK3), follow=0x37)
    C("content-length 18 digits", REQ, P3 + [F(CL, b"1" * 18)], E(0, "0000", content_length=111111111111111111, **OK3),
      follow=0x39)
    C("content-length 19 nines", REQ, P3 + [F(CL, b"9999999999999999999")],
      E(0, "0000", content_length=9999999999999999999, **OK3), follow=0x39)
    C("content-length 19 digits, leading zeros", REQ, P3 + [F(CL, b"0000000000000000001")],
      E(0, "0000", content_length=1, **OK3), follow=0x30)
    C("content-length 20 digits", REQ, P3 + [F(CL, b"18446744073709551615")], E(-1, "0000", err=5, **OK3))
    C("content-length 20 zeros", REQ, P3 + [F(CL, b"0" * 20)], E(-1, "0000", err=5, **OK3))
    C("content-length +1", REQ, P3 + [F(CL, b"+1")], E(-1, "0000", err=5, **OK3))
    C("content-length leading space", REQ, P3 + [F(CL, b" 1", 2)], E(-1, "0000", err=5, **OK3))
    C("content-length trailing space", REQ, P3 + [F(CL, b"1 ", 2)], E(-1, "0000", err=5, **OK3))
    C("content-length 12a", REQ, P3 + [F(CL, b"12a")], E(-1, "0000", err=5, **OK3))
    C("content-length a12", REQ, P3 + [F(CL, b"a12")], E(-1, "0000", err=5, **OK3))
    C("content-length digit with the high bit", REQ, P3 + [F(CL, b"1\xb2")], E(-1, "0000", err=5, **OK3))
    C("content-length slash", REQ, P3 + [F(CL, b"1"), F(CL, b"/")], E(-1, "00000", err=5, content_length=NO_LENGTH, **OK3))
    C("content-length colon", REQ, P3 + [F(CL, b":")], E(-1, "0000", err=5, **OK3))
    C("content-length twice", REQ, P3 + [F(CL, b"5"), F(b"date"), F(CL, b"6")],
      E(0, "000010", content_length=6, **OK3))
    C("content-length good then bad", REQ, P3 + [F(CL, b"5"), F(CL, b"x")], E(-1, "00000", err=5, **OK3))
    C("content-length in a response", HEAD, [S200, F(CL, b"12a"), F(CL, b"")], E(0, "011", status=200))
    C("content-length in trailers", TRAILERS, [F(CL, b"12a")], E(0, "1"))
    # ---- limits (:528-532, :621-631) -----------------------------------------------------------------
    C("100 listed", REQ, P3 + [DATE] * 100, E(0, "000" + "1" * 100, **OK3))
    C("101st not listed", REQ, P3 + [DATE] * 101 + [F(b"x-after", b"v")],
      E(SOFT, "000" + "1" * 100 + "00", err=3, **OK3), at=103)
    C("101st after a soft name error", REQ, P3 + [F(b"x b", b"v", 1)] + [DATE] * 100,
      E(SOFT, "000" + "1" * 100 + "0", err=1, **OK3))
    C("not counted towards the 100", H3_REQ,
      [GET, HTTPS, ROOT, F(b":authority", b"a"), F(b":protocol", b"p"), F(b"host", b"h"), F(b"expect", b"x"),
       F(CL, b"1"), F(b"datagram-flow-id", b"4")] + [DATE] * 100,
      E(0, "0" * 9 + "1" * 100, method=0, scheme=1, path=2, authority=3, protocol=4, expect=6, content_length=1,
        datagram_flow_id=8, exists_map=31, scheme_kind=2))
    C("not counted towards the 100", H2_REQ,
      [GET, HTTPS, ROOT, F(b":authority", b"a"), F(b":protocol", b"p"), F(b"host", b"h"), F(b"expect", b"x"),
       F(CL, b"1"), F(b"datagram-flow-id", b"4")] + [DATE] * 100,
      E(0, "0" * 9 + "1" * 100, method=0, scheme=1, path=2, authority=3, protocol=4, expect=6, content_length=1,
        exists_map=31, scheme_kind=2))
    C("100 listed in a response", HEAD, [S200] + [DATE] * 100, E(0, "0" + "1" * 100, status=200))
    C("101st in a response", HEAD, [S200] + [DATE] * 101, E(SOFT, "0" + "1" * 100 + "0", status=200, err=3))
    C("101st in trailers", TRAILERS, [DATE] * 101, E(SOFT, "1" * 100 + "0", err=3))
    C("flow id not counted in a response", H3_RES, [S200, F(b"datagram-flow-id", b"4")] + [DATE] * 100,
      E(0, "00" + "1" * 100, status=200, datagram_flow_id=1))
    C("1000 fields", REQ, P3 + [DATE] * 997, E(SOFT, "000" + "1" * 100 + "0" * 897, err=3, **OK3))
    C("1001 fields", REQ, P3 + [DATE] * 998, E(-9, "000" + "1" * 100 + "0" * 898, err=3, **OK3))
    C("1000 fields in a response", HEAD, [S200] + [DATE] * 999, E(SOFT, "0" + "1" * 100 + "0" * 899, status=200, err=3))
    C("1001 fields in a response", HEAD, [S200] + [DATE] * 1000,
      E(-9, "0" + "1" * 100 + "0" * 900, status=200, err=3))
    C("1000 fields in trailers", TRAILERS, [DATE] * 1000, E(SOFT, "1" * 100 + "0" * 900, err=3))
    C("1001 fields in trailers", TRAILERS, [DATE] * 1001, E(-9, "1" * 100 + "0" * 901, err=3))
    C("1001st is a bad content-length", REQ, P3 + [DATE] * 997 + [F(CL, b"x")],
      E(-9, "000" + "1" * 100 + "0" * 898, err=3, **OK3))
    C("1000th is a bad content-length", REQ, P3 + [DATE] * 996 + [F(CL, b"x")],
      E(-1, "000" + "1" * 100 + "0" * 897, err=5, **OK3))
    # ---- request pseudo-headers (:533-586) -----------------------------------------------------------
    C(":method twice", REQ, [GET, F(b":method", b"POST")], E(-1, "00", err=4, method=0, exists_map=1))
    C(":scheme twice", REQ, [F(b":scheme", b"http"), HTTPS], E(-1, "00", err=4, scheme=0, exists_map=2, scheme_kind=1))
    C(":path twice", REQ, [ROOT, F(b":path", b"/index.html")], E(-1, "00", err=4, path=0, exists_map=4))
    C(":authority twice", REQ, [F(b":authority", b"a"), F(b":authority", b"")], E(-1, "00", err=4, authority=0, exists_map=8))
    C(":protocol twice", REQ, [F(b":protocol", b"websocket"), F(b":protocol", b"websocket")],
      E(-1, "00", err=0, protocol=0, exists_map=16))
    C(":protocol twice after a soft error", REQ, [F(b":protocol", b"a\x01", 2), F(b":protocol", b"b")],
      E(-1, "00", err=2, protocol=0, exists_map=16))
    C("empty :path", REQ, [GET, F(b":path", b"")], E(-1, "00", err=4, method=0, exists_map=1))
    C("empty :authority", REQ, [F(b":authority", b"")], E(0, "0", authority=0, exists_map=8))
    C(":status in a request", REQ, [GET, S200], E(-1, "00", err=0, method=0, exists_map=1))
    Cp(":foo in a request", H2_REQ, H3_REQ, lambda soft: [GET, F(b":foo", b"bar", soft)],
       E(-1, "00", err=0, method=0, exists_map=1), E(-1, "00", err=1, method=0, exists_map=1))
    Cp("the name ':' alone", H2_REQ, H3_REQ, lambda soft: [GET, F(b":", b"x", soft)],
       E(-1, "00", err=0, method=0, exists_map=1), E(-1, "00", err=1, method=0, exists_map=1))
    C("pseudo-header after a regular field", REQ, [GET, DATE, ROOT], E(-1, "010", err=4, method=0, exists_map=1))
    Cp("unknown pseudo-header after a regular field", H2_REQ, H3_REQ, lambda soft: [GET, DATE, F(b":foo", b"x", soft)],
       E(-1, "010", err=4, method=0, exists_map=1))
    C("pseudo-headers in reverse order", REQ,
      [F(b":protocol", b"p"), F(b":authority", b"a"), F(b":path", b"/index.html"), F(b":scheme", b"http"),
       F(b":method", b"POST")],
      E(0, "00000", protocol=0, authority=1, path=2, scheme=3, method=4, exists_map=31, scheme_kind=1))
    C("pseudo-headers, a subset out of order", REQ, [ROOT, F(b":authority", b"a"), GET, DATE],
      E(0, "0001", path=0, authority=1, method=2, exists_map=13))
    for bit, fld, key in ((1, GET, "method"), (2, HTTPS, "scheme"), (4, ROOT, "path"), (8, F(b":authority", b"a"), "authority"),
                          (16, F(b":protocol", b"p"), "protocol")):
        C("%s alone" % fld[0].decode(), REQ, [fld],
          E(0, "0", exists_map=bit, **dict({key: 0}, **({"scheme_kind": 2} if bit == 2 else {}))))
    C("no field at all", REQ, [], E(0, ""))
    for value, kind in ((b"http", 1), (b"https", 2), (b"masque", 3), (b"HTTPS", 1), (b"httpx", 1), (b"", 1),
                        (b"masqu", 1), (b"masquee", 1)):
        C(":scheme %r" % value.decode(), REQ, [F(b":scheme", value)], E(0, "0", scheme=0, exists_map=2, scheme_kind=kind),
          follow={b"http": 0x73, b"masqu": 0x65}.get(value))
    # ---- host / :authority (:536-542, :601-605) ------------------------------------------------------
    C("host alone", REQ, P3 + [F(b"host", b"h.example")], E(0, "0000", authority=3, **OK3))
    C("host with the static table's empty value", REQ, P3 + [F(b"host", b"")], E(0, "0000", authority=3, **OK3))
    C(":authority then host", REQ, [F(b":authority", b"a"), F(b"host", b"h")], E(0, "00", authority=0, exists_map=8))
    C("host twice", REQ, [GET, F(b"host", b"one"), F(b"host", b"two")], E(0, "000", method=0, authority=1, exists_map=1))
    C("host then :authority", REQ, [F(b"host", b"h"), F(b":authority", b"a")], E(-1, "00", err=4, authority=0))
    C("host in a response", HEAD, [S200, F(b"host", b"h")], E(0, "01", status=200))
    C("host in trailers", TRAILERS, [F(b"host", b"h")], E(0, "1"))
    # ---- te (:606, h2o_lcstris) ---------------------------------------------------------------------
    for value, ok, follow in ((b"trailers", 1, None), (b"TRAILERS", 1, None), (b"tRaIlErS", 1, None), (b"trailer", 0, 0x73),
                              (b"trailers ", 0, None), (b"trailerz", 0, None), (b"", 0, None), (b"gzip", 0, None),
                              (b"@railers", 0, None), (b"[railers", 0, None), (b"trailer@", 0, None),
                              (b"`railers", 0, None), (b"{railers", 0, None), (b"\xf4railers", 0, None),
                              (b"trailers, deflate", 0, None), (b"railers", 0, None)):
        soft = 2 if value.endswith(b" ") else 0
        C("te %r" % value, REQ, P3 + [F(b"te", value, soft)],
          E(0, "0001", **OK3) if ok else E(-1, "0000", err=6, **OK3), follow=follow)
    C("te trailers in a response", HEAD, [S200, F(b"te", b"trailers")], E(-1, "00", status=200, err=6))
    C("te trailers in trailers", TRAILERS, [F(b"te", b"trailers")], E(-1, "0", err=6))
    # ---- names one edit away from every class (req_name_class) ----------------------------------------
    near = [b"tf", b"ue", b"t", b"tes", b"hosu", b"iost", b"hos", b"hostt", b"expecu", b"fxpect", b"expec", b"expectt",
            b"upgradf", b"vpgrade", b"upgrad", b"upgradee", b"connectioo", b"donnection", b"connectio", b"connectionn",
            b"cache-digesu", b"dache-digest", b"cache-diges", b"cache-digestt", b"content-lengti", b"dontent-length",
            b"content-lengt", b"content-lengthh", b"http2-settingt", b"ittp2-settings", b"http2-setting",
            b"http2-settingss", b"datagram-flow-ie", b"eatagram-flow-id", b"datagram-flow-i", b"datagram-flow-idd",
            b"transfer-encodinh", b"uransfer-encoding", b"transfer-encodin", b"transfer-encodingg"]
    for n in near:
        C("near name %s in a request" % n.decode(), REQ, P3 + [F(n, b"12a")], E(0, "0001", **OK3))
        C("near name %s in a response" % n.decode(), HEAD, [S200, F(n, b"12a")], E(0, "01", status=200))
    for n in (b":patg", b":qath", b":pat", b":pathh", b":methoe", b":nethod", b":metho", b":methodd", b":schemf",
              b":tcheme", b":schem", b":schemee", b":statut", b":ttatus", b":statu", b":statuss", b":protocom",
              b":qrotocol", b":protoco", b":protocoll", b":authoritz", b":buthority", b":authorit", b":authorityy"):
        Cp("near pseudo name %s in a request" % n.decode(), H2_REQ, H3_REQ, lambda soft, n=n: [GET, F(n, b"/", soft)],
           E(-1, "00", err=0, method=0, exists_map=1), E(-1, "00", err=1, method=0, exists_map=1))
        Cp("near pseudo name %s in a response" % n.decode(), H2_RES, H3_RES, lambda soft, n=n: [F(n, b"200", soft)],
           E(-1, "0", err=4))
    # an upper-case letter behind the colon: an unknown pseudo-header, but refused by QPACK's raw literal
    C(":Path in a request", H2_REQ, [GET, F(b":Path", b"/")], E(-1, "00", err=0, method=0, exists_map=1))
    C(":Path in a request, raw in QPACK", H3_REQ, [GET, F(b":Path", b"/", UPPER)], E(-1, "0", err=7, method=0, exists_map=1))
    C(":Path in a request, Huffman in QPACK", H3_REQ, [GET, F(b":Path", b"/")], E(-1, "00", err=0, method=0, exists_map=1),
      routes=("lit_huff",))
    C(":Status in a response", H2_RES, [F(b":Status", b"200")], E(-1, "0", err=4))
    C(":Status in a response, raw in QPACK", H3_RES, [F(b":Status", b"200", UPPER)], E(-1, "", err=7))
    C(":Status in a response, Huffman in QPACK", H3_RES, [F(b":Status", b"200")], E(-1, "0", err=4), routes=("lit_huff",))
    # ---- per-protocol differences (:598-619) ---------------------------------------------------------
    C("cache-digest in h2", H2_REQ, P3 + [F(b"cache-digest", b"AfdA")], E(0, "0001", **OK3))
    C("cache-digest in h3", H3_REQ, P3 + [F(b"cache-digest", b"AfdA")], E(-1, "0000", err=6, **OK3))
    C("cache-digest in a response", HEAD, [S200, F(b"cache-digest", b"AfdA")], E(0, "01", status=200))
    C("cache-digest in trailers", TRAILERS, [F(b"cache-digest", b"AfdA")], E(0, "1"))
    C("datagram-flow-id in h2", H2_REQ, P3 + [F(b"datagram-flow-id", b"4"), F(b"datagram-flow-id", b"8")],
      E(0, "00000", **OK3))
    C("datagram-flow-id in h3", H3_REQ, P3 + [F(b"datagram-flow-id", b"4"), F(b"datagram-flow-id", b"8")],
      E(0, "00000", datagram_flow_id=4, **OK3))
    C("datagram-flow-id in an h2 response", H2_RES, [S200, F(b"datagram-flow-id", b"4"), F(b"datagram-flow-id", b"8")],
      E(0, "000", status=200))
    C("datagram-flow-id in an h3 response", H3_RES, [S200, F(b"datagram-flow-id", b"4"), F(b"datagram-flow-id", b"8")],
      E(0, "000", status=200, datagram_flow_id=2))
    C("datagram-flow-id in trailers", TRAILERS, [F(b"datagram-flow-id", b"4"), DATE], E(0, "01"))
    C("expect", REQ, P3 + [F(b"expect", b"100-continue"), DATE, F(b"expect", b"")], E(0, "000010", expect=5, **OK3))
    for n in (b"connection", b"upgrade", b"http2-settings", b"transfer-encoding"):
        C("%s in a request" % n.decode(), REQ, P3 + [DATE, F(n, b"trailers")], E(-1, "00010", err=6, **OK3))
        C("%s in a response" % n.decode(), HEAD, [S200, DATE, F(n, b"trailers")], E(-1, "010", status=200, err=6))
        C("%s in trailers" % n.decode(), TRAILERS, [DATE, F(n, b"trailers")], E(-1, "10", err=6))
    # ---- response heads (:652-709) -------------------------------------------------------------------
    for value, verdict, status, follow in ((b"200", 0, 200, None), (b"100", 0, 100, None), (b"999", 0, 999, None),
                                           (b"099", -1, 0, None), (b"20", -1, 0, 0x30), (b"1000", -1, 0, None),
                                           (b"2x0", -1, 200, None), (b"20x", -1, 200, None), (b"x00", -1, 0, None),
                                           (b"29:", -1, 290, None), (b"2/0", -1, 200, None), (b":00", -1, 0, None),
                                           (b"/00", -1, 0, None), (b"2\xb00", -1, 200, None), (b"", -1, 0, None),
                                           (b"204", 0, 204, None), (b"206", 0, 206, None), (b"304", 0, 304, None),
                                           (b"400", 0, 400, None), (b"404", 0, 404, None), (b"500", 0, 500, None)):
        C(":status %r" % value, HEAD, [F(b":status", value)],
          E(0, "0", status=status) if verdict == 0 else E(-1, "0", status=status, err=4), follow=follow)
    C(":status twice", HEAD, [S200, S200], E(-1, "00", status=200, err=4))
    C(":status after a field", HEAD, [S200, DATE, S200], E(-1, "010", status=200, err=4))
    C("a regular field before :status", HEAD, [DATE, S200], E(-1, "0", err=9))
    C(":path in a head", HEAD, [ROOT], E(-1, "0", err=4))
    for n in (b":method", b":scheme", b":protocol", b":authority"):
        C("%s in a head" % n.decode(), HEAD, [F(n, b"x")], E(-1, "0", err=4))
        C("%s in trailers" % n.decode(), TRAILERS, [F(n, b"x")], E(-1, "0", err=4))
    C(":path after :status", HEAD, [S200, ROOT], E(-1, "00", status=200, err=4))
    C("an empty head", HEAD, [], E(-1, "", err=9))
    C("expect in a response", HEAD, [S200, F(b"expect", b"100-continue")], E(-1, "00", status=200, err=6))
    C("accept-encoding listed", REQ, P3 + [F(b"accept-encoding", b"gzip, deflate")], E(0, "0001", **OK3))
    C(":method POST, :path /index.html, :scheme http", REQ,
      [F(b":method", b"POST"), F(b":path", b"/index.html"), F(b":scheme", b"http"), DATE],
      E(0, "0001", method=0, path=1, scheme=2, exists_map=7, scheme_kind=1))
    # ---- trailers (:679-682) ---------------------------------------------------------------------------
    C(":status in trailers", TRAILERS, [S200], E(-1, "0", err=4))
    C(":status after a field in trailers", TRAILERS, [DATE, S200], E(-1, "10", err=4))
    C(":path in trailers", TRAILERS, [ROOT], E(-1, "0", err=4))
    C("trailers", TRAILERS, [DATE, F(b"x-checksum", b"abc")], E(0, "11"))
    C("empty trailers", TRAILERS, [], E(-9, ""))
    C("expect in trailers", TRAILERS, [F(b"expect", b"x")], E(-1, "0", err=6))
    # ---- ordering of soft and hard errors (:518-527) ---------------------------------------------------
    C("soft value error, then a hard rule error", REQ, P3 + [F(b"x-a", b"\x01v", 2), F(CL, b"x")],
      E(-1, "00010", err=5, **OK3))
    Cp("soft value error, then an unknown pseudo-header", H2_REQ, H3_REQ,
       lambda soft: [F(b":method", b"G\x01T", 2), F(b":foo", b"x", soft)], E(-1, "00", err=2, method=0, exists_map=1))
    C("soft value error alone", REQ, P3 + [F(b"x-a", b"\x01v", 2), DATE], E(SOFT, "00011", err=2, **OK3), at=3)
    C("soft name error alone", REQ, P3 + [F(b"x b", b"v", 1)], E(SOFT, "0001", err=1, **OK3))
    C("soft value, then soft name", REQ, P3 + [F(b"x-a", b"v\x7f", 2), F(b"x b", b"v", 1)], E(SOFT, "00011", err=2, **OK3))
    C("soft name, then soft value", REQ, P3 + [F(b"x b", b"v", 1), F(b"x-a", b"v\x7f", 2)], E(SOFT, "00011", err=1, **OK3))
    C("soft name and value in one field", REQ, P3 + [F(b"x b", b"\x01", 3)], E(SOFT, "0001", err=1, **OK3))
    C("soft error on the decisive content-length", REQ, P3 + [F(CL, b"1\x01", 2)], E(-1, "0000", err=5, **OK3))
    C("soft value error in a response, then a hard one", HEAD, [S200, F(b"x-a", b"\x01v", 2), F(b"te", b"trailers")],
      E(-1, "010", status=200, err=6))
    C("soft value error alone in a response", HEAD, [S200, F(b"x-a", b"v\t", 2)], E(SOFT, "01", status=200, err=2))
    C("soft value error alone in trailers", TRAILERS, [F(b"x-a", b"v\t", 2)], E(SOFT, "1", err=2))
    C("soft error on :status", HEAD, [F(b":status", b"20\x01", 2)], E(-1, "0", status=200, err=4))
    C("upper-case literal name", REQ, P3 + [F(b"Upper", b"v", UPPER)], E(-1, "000", err=7, **OK3))
    C("upper-case literal name after a soft error", REQ, P3 + [F(b"x b", b"v", 1), F(b"x-Upper", b"v", UPPER)],
      E(-1, "0001", err=7, **OK3))
    C("upper-case literal name in a response", HEAD, [S200, F(b"Upper", b"v", UPPER)], E(-1, "0", status=200, err=7))
    C("upper-case literal name in trailers", TRAILERS, [DATE, F(b"Te", b"v", UPPER)], E(-1, "1", err=7))
    names = [(k["name"], p) for k in out for p in k["parsers"]]
    assert len(names) == len(set(names)), [n for n in names if names.count(n) > 1]
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return _cases()


def cases_for(parser):
    return [k for k in cases() if parser in k["parsers"]]


# ------------------------------------------------------------------------------------------------
# HPACK: the wire
# ------------------------------------------------------------------------------------------------
RAW = lambda s: string(s, False)  # noqa: E731
HUF = lambda s: string(s, True)  # noqa: E731
H_MODE = {"h2_req": "req", "h2_res": "res", "h2_trailers": "res"}
# a value every rule accepts for the name, to insert it in the mode under test
OK_VALUE = {b"te": b"trailers", b"content-length": b"1", b":path": b"/", b":status": b"200", b":scheme": b"http"}


def _h_static(name, value=None):
    """the HPACK static index of the pair (value None: of the name), or 0"""
    for i, (n, v) in enumerate(HSTATIC):
        if n == name and (value is None or v == value):
            return i + 1
    return 0


def h_field(fld):
    """a field by its default route: a static index, a static name index, or raw literals; never inserted"""
    name, value, _ = fld
    if _h_static(name, value):
        return indexed(_h_static(name, value))
    if _h_static(name):
        return literal(_h_static(name), RAW(value), "without")
    return literal(RAW(name), RAW(value), "without")


def h_block(fields, at=None, wire=None):
    return b"".join(wire if k == at else h_field(f) for k, f in enumerate(fields))


def _guard(follow):
    g = bytes([follow if follow is not None else 0x7A]) * 2
    return (g, g, 0)


def _h_setup(parser, fld, follow):
    """-> (the fields of a block that inserts `fld` between two guard entries, fld's position among them): the block
    starts as its parser requires, and a pseudo-header comes before the guards"""
    g = _guard(follow)
    pseudo = fld[0][:1] == b":"
    head = [S200] if parser == "h2_res" and not pseudo else []
    body = [fld, g, g] if pseudo else [g, fld, g]
    return head + body, len(head) + (0 if pseudo else 1)


def _h_setup_block(fields, first_inserted):
    return b"".join(h_field(f) if k < first_inserted else literal(RAW(f[0]), RAW(f[1]), "inc")
                    for k, f in enumerate(fields))


def hpack_variants(parser):
    """-> ([variant], [(case, route, why not)]); a variant: dict(name, case, route, plan ("same": every call in the
    parser's mode, "plain": the first call in plain mode), conns (per call the blocks of the case's connection),
    where (call, block) of the case's block, trailers {(call, block)}, follow)"""
    import rules_model as RM

    out, unreachable = [], []
    for k in cases_for(parser):
        fields, at, follow = k["fields"], k["at"], k["follow"]
        tr = parser == "h2_trailers"

        def add(route, plan, calls, where):
            flags = {(i, b) for i, blocks in enumerate(calls) for b in range(len(blocks))} if tr else set()
            out.append(dict(name="%s | %s | %s" % (parser, k["name"], route), case=k, route=route, plan=plan, conns=calls,
                            where=where, trailers=flags, follow=follow))

        if not fields:
            add("empty", "same", [[b""]], (0, 0))
            continue
        name, value, soft = fields[at]
        add("lit_raw", "same", [[h_block(fields, at, literal(RAW(name), RAW(value), "without"))]], (0, 0))
        if soft == UPPER:
            unreachable.append((k["name"], "every table route", "an upper-case name never enters a table"))
            continue
        add("lit_huff", "same", [[h_block(fields, at, literal(HUF(name), HUF(value), "never"))]], (0, 0))
        if soft:
            unreachable.append((k["name"], "table routes", "soft-error bits belong to the literal"))
            continue
        if _h_static(name, value):
            add("static_idx", "same", [[h_block(fields, at, indexed(_h_static(name, value)))]], (0, 0))
        else:
            unreachable.append((k["name"], "static_idx", "the pair is not in the static table"))
        if _h_static(name):
            add("static_ref", "same", [[h_block(fields, at, literal(_h_static(name), RAW(value), "without"))]], (0, 0))
        # the entry's index in the case's block: the setup leaves it second-newest (63) or, a pseudo-header, oldest (64)
        idx = 64 if name[:1] == b":" else 63
        by_idx, by_ref = h_block(fields, at, indexed(idx)), h_block(fields, at, literal(idx, RAW(value), "without"))
        for what, entry in (("idx", fields[at]), ("ref", (name, OK_VALUE.get(name, b"x"), 0))):
            setup, first = _h_setup(parser, entry, follow)
            block = by_idx if what == "idx" else by_ref
            if RM.parse(setup, parser)["verdict"] == 0:
                add("same_" + what, "same", [[_h_setup_block(setup, first), block]], (0, 1))
                add("earlier_" + what, "same", [[_h_setup_block(setup, first)], [block]], (1, 0))
            else:
                unreachable.append((k["name"], "same_%s, earlier_%s" % (what, what),
                                    "the inserting block is a hard error in this mode"))
            plain, first = _h_setup("h2_trailers", entry, follow)  # no rules in plain mode: no head needed
            add("plain_" + what, "plain", [[_h_setup_block(plain, first)], [block]], (1, 0))
    return out, unreachable


def _follower(follow):
    return bytes([follow, 0x00])  # its first byte is what the rule would accept next; whatever it decodes to


def hpack_corpus(variants, plan):
    """the variants of one plan as a blocks_harness corpus of two calls: every variant a connection, followed (where
    the case names a follow byte) by a connection whose block in the same call starts with that byte"""
    cs = []
    for v in variants:
        if v["plan"] != plan:
            continue
        conns = [v["conns"] + [[]] * (2 - len(v["conns"]))]
        if v["follow"] is not None:
            conns.append([[_follower(v["follow"])] if i == v["where"][0] else [] for i in range(2)])
        cs.append(ccase(v["name"], *conns, trailers={(0, i, b) for i, b in v["trailers"]}))
    return cs


def interleave(variants, key):
    """an order in which neighbouring lanes take different branches: accepting and failing cases alternate as far as
    they last"""
    ok = [v for v in variants if key(v) == 0]
    bad = [v for v in variants if key(v) != 0]
    out = []
    while ok or bad:
        if ok:
            out.append(ok.pop(0))
        if bad:
            out.append(bad.pop(0))
    return out


def hpack_batches(mode):
    """-> [(label, batch, modes, [(variant, parser)])]: for hhuff_hpack_parse_requests (mode "req") or _responses
    ("res": heads and trailers in one call) every case by every route, one batch per plan"""
    from blocks_harness import batch

    parsers = [p for p, m in H_MODE.items() if m == mode]
    vs = [(v, p) for p in parsers for v in hpack_variants(p)[0]]
    out = []
    for plan, modes in (("same", [mode, mode]), ("plain", ["plain", mode])):
        mine = interleave([vp for vp in vs if vp[0]["plan"] == plan], lambda vp: expect_for(vp[0]["case"], vp[1])["verdict"])
        bt = batch(hpack_corpus([v for v, _ in mine], plan), 4096, spacers=False, arena_base=19, tail=1)
        out.append(("rules %s %s" % (mode, plan), bt, modes, mine))
    return out


def filler(parser):
    """a connection that is accepted, for the lanes around a case that is alone"""
    if parser.endswith("req"):
        return P3 + [DATE]
    return [DATE] if parser == "h2_trailers" else [S200, DATE]


def hpack_alone_batches(mode):
    """every case by its lit_raw route at connections 0, 63 and 64 of a 65-connection batch of accepted connections"""
    from blocks_harness import batch

    out = []
    for p in [p for p, m in H_MODE.items() if m == mode]:
        fill = h_block(filler(p))
        for v in hpack_variants(p)[0]:
            if v["route"] not in ("lit_raw", "empty"):
                continue
            tr = {(0, 0)} if p == "h2_trailers" else set()
            one = lambda i: ccase("%s @%d" % (v["name"], i), v["conns"], trailers={(0, c, b) for c, b in tr})  # noqa: E731
            fl = [ccase("filler %d" % i, [[fill]], trailers={(0, c, b) for c, b in tr}) for i in range(62)]
            bt = batch([one(0)] + fl + [one(63), one(64)], 4096, spacers=False)
            out.append(("%s alone" % v["name"], bt, [mode], [(dict(v, name="%s @%d" % (v["name"], i)), p) for i in (0, 63, 64)]))
    return out


# ------------------------------------------------------------------------------------------------
# QPACK: the wire
# ------------------------------------------------------------------------------------------------
QV = lambda s, h=False: qstr(huffman(s) if h else s, 7, 0, h)  # noqa: E731
Q_MODE = {"h3_req": "qreq", "h3_res": "qres"}
HTS = 4096


def _q_static(name, value=None):
    for i, (n, v) in enumerate(QSTATIC):
        if n == name and (value is None or v == value):
            return i
    return -1


def q_field(fld):
    name, value, _ = fld
    if _q_static(name, value) >= 0:
        return q_indexed(_q_static(name, value), True)
    if _q_static(name) >= 0:
        return q_literal_ref(_q_static(name), QV(value), True)
    return q_literal(name, QV(value))


def q_section(fields, at=None, wire=None, ric=0, base=0):
    return q_prefix(ric, base, HTS // 32) + b"".join(wire if k == at else q_field(f) for k, f in enumerate(fields))


def qpack_variants(parser):
    """-> ([variant], unreachable): dict(name, case, route, enc (the step's encoder stream), section, follow)"""
    out, unreachable = [], []
    for k in cases_for(parser):
        fields, at, follow = k["fields"], k["at"], k["follow"]

        def add(route, section, enc=b""):
            out.append(dict(name="%s | %s | %s" % (parser, k["name"], route), case=k, route=route, enc=enc,
                            section=section, follow=follow))

        if not fields:
            add("empty", q_section([]))
            continue
        name, value, soft = fields[at]
        g = _guard(follow)
        ins = lambda f: q_insert(f[0], QV(f[1]))  # noqa: E731
        whole = ins(g) + ins(fields[at]) + ins(g)  # absolute indices 0, 1, 2: the encoder stream has no rules
        named = ins(g) + ins((name, b"x", 0)) + ins(g)
        can = {"lit_raw": (q_literal(name, QV(value)), 0, 0, b""),
               "lit_huff": (q_literal(huffman(name), QV(value, True), True, never=True), 0, 0, b""),
               "dyn_idx": (q_indexed(1), 3, 3, whole), "post_idx": (q_indexed_post(1), 3, 0, whole),
               "dyn_ref": (q_literal_ref(1, QV(value)), 3, 3, named),
               "post_ref": (q_literal_post(1, QV(value, True)), 3, 0, named)}
        if _q_static(name, value) >= 0:
            can["static_idx"] = (q_indexed(_q_static(name, value), True), 0, 0, b"")
        if _q_static(name) >= 0:
            can["static_ref"] = (q_literal_ref(_q_static(name), QV(value), True), 0, 0, b"")
        if k["routes"] is not None:  # the case says by which routes its field arrives as the case describes it
            take = k["routes"]
        elif soft == UPPER:
            take = ("lit_raw",)
            unreachable.append((k["name"], "every table route", "an upper-case name never enters a table"))
        elif soft:
            take = ("lit_raw", "lit_huff")
            unreachable.append((k["name"], "table routes", "soft-error bits belong to the literal"))
        else:
            take = tuple(can)
            if "static_idx" not in can:
                unreachable.append((k["name"], "static_idx", "the pair is not in the static table"))
        for route in take:
            wire, ric, base, enc = can[route]
            add(route, q_section(fields, at, wire, ric, base), enc)
    return out, unreachable


def _qconns(v):
    conns = [[(v["enc"], [v["section"]])]]
    if v["follow"] is not None:
        conns.append([(b"", [_follower(v["follow"])])])
    return conns


def qpack_batches(parser):
    """-> [(label, session, mode, [(variant, parser)])]: every case by every route in one step"""
    from blocks_harness import qbatch

    vs = interleave([(v, parser) for v in qpack_variants(parser)[0]],
                    lambda vp: expect_for(vp[0]["case"], parser)["verdict"])
    bt = qbatch([qcase(v["name"], *_qconns(v)) for v, _ in vs], HTS, 2, spacers=False, arena_base=21)
    return [("rules %s" % parser, bt, Q_MODE[parser], vs)]


def qpack_alone_batches(parser):
    from blocks_harness import qbatch

    fill = q_section(filler(parser))
    out = []
    for v in qpack_variants(parser)[0]:
        if v["route"] not in ("lit_raw", "empty"):
            continue
        one = lambda i: qcase("%s @%d" % (v["name"], i), [(b"", [v["section"]])])  # noqa: E731
        bt = qbatch([one(0)] + [qcase("filler %d" % i, [(b"", [fill])]) for i in range(62)] + [one(63), one(64)], HTS, 2,
                    spacers=False)
        out.append(("%s alone" % v["name"], bt, Q_MODE[parser], [(dict(v, name="%s @%d" % (v["name"], i)), parser)
                                                                  for i in (0, 63, 64)]))
    return out


# ------------------------------------------------------------------------------------------------
# the literal expectations against a summary (blocks_harness.summary / qsummary)
# ------------------------------------------------------------------------------------------------
def block_of(cl, v, hpack):
    """the index, in a call / step, of the variant's own block"""
    if hpack:
        return cl["labels"].index("%s[call %d block %d]" % ((v["name"],) + v["where"]))
    return cl["labels"].index("%s[step 0 section 0]" % v["name"])


def check_literal(summary, bt, modes, variants, label=""):
    """every variant's block in the summary (of the restatement, the reference, the fixture or the GPU) against the
    case's literal expectation: verdict, number of fields, header flags, soft bits, record words"""
    import numpy as np

    hpack = isinstance(modes, list)
    for v, parser in variants:
        i = v["where"][0] if hpack else 0
        mode = modes[i] if hpack else modes
        b = block_of(bt["calls"][i], v, hpack)
        e = expect_for(v["case"], parser)
        where = "%s: %s" % (label, v["name"])
        nf = summary["%d_nfields" % i]
        assert int(summary["%d_bstatus" % i][b]) == e["verdict"], "%s: verdict %d, expected %d" % (
            where, summary["%d_bstatus" % i][b], e["verdict"])
        assert int(nf[b]) == e["nfields"], "%s: %d fields, expected %d" % (where, nf[b], e["nfields"])
        s = int(nf[:b].astype(np.int64).sum())
        got = (summary["%d_header" % i][s:s + e["nfields"]] != 0).astype(int).tolist()
        assert got == e["header"], "%s: header flags %s, expected %s" % (where, got, e["header"])
        soft = [f[2] for f in v["case"]["fields"][:e["nfields"]]]
        got = summary["%d_soft" % i][s:s + e["nfields"]].tolist()
        assert got == [1 if x & 1 else 2 if x & 2 else 0 for x in soft], "%s: soft codes %s" % (where, got)
        want = record_words(e["rec"], parser)
        got = summary["%d_%s" % (i, mode)][b][:len(want)].tolist()
        assert got == want, "%s: record %s, expected %s" % (where, got, want)


def fixture_key(label, key):
    return "%s|%s" % (label, key)


def reference_results(codec):
    """the arrays of tests/golden/rule_edges.npz (oracle/gen_golden.py): every batch of every case and route through
    `codec`, the compiled reference: statuses, field counts, header flags, soft codes and records.  The fields' bytes
    are left out (block_edges.npz pins the decoders); the 1000-field cases make them large."""
    import blocks_harness as BH

    out = {}
    keep = lambda k: not k.endswith(("_name", "_value", "_name_len", "_value_len"))  # noqa: E731
    for mode in ("req", "res"):
        for label, bt, modes, _ in hpack_batches(mode):
            for k, a in BH.summary(BH.expected(codec, bt, modes), bt, modes).items():
                if keep(k):
                    out[fixture_key(label, k)] = a
    for parser in Q_MODE:
        for label, bt, mode, _ in qpack_batches(parser):
            for k, a in BH.qsummary(BH.qexpected(codec, bt, mode), bt, mode).items():
                if keep(k):
                    out[fixture_key(label, k)] = a
    return out
