"""rpkt_gpu_coalesce_batch on the CPU: tests/coalesce_model.py (the model the GPU test compares
bytes against) anchored to the oracle's parse, to segmentation (coalesce(segment(F)) == F)
and to one case per rule that breaks or keeps a link; engine.flow_order on CPU tensors."""
import numpy as np
import pytest

from rpkt_amd import engine

import coalesce_model as cm
import segment_model as sm

ACK, PSH, FIN, CWR = sm.ACK, sm.PSH, sm.FIN, sm.CWR


def fix_tcp4(f, l3=14):
    """`f` (Ether / IPv4 / TCP) with its TCP checksum recomputed."""
    f = bytearray(f)
    ihl = (f[l3] & 15) * 4
    l4, tot = l3 + ihl, int.from_bytes(f[l3 + 2:l3 + 4], "big")
    f[l4 + 16:l4 + 18] = b"\0\0"
    pseudo = bytes(f[l3 + 12:l3 + 20]) + b"\0\x06" + (tot - ihl).to_bytes(2, "big")
    f[l4 + 16:l4 + 18] = sm.csum_field(pseudo, f[l4:l3 + tot]).to_bytes(2, "big")
    return bytes(f)


def patched(f, at, value):
    f = bytearray(f)
    f[at:at + len(value)] = value
    return fix_tcp4(f)


def stream(sizes, seq=1000, ident=7, flags=ACK, salt=0, **kw):
    """Consecutive segments of one flow: payload sizes, seq and ident running on."""
    out = []
    for k, p in enumerate(sizes):
        out.append(sm.tcp4(sm.payload_bytes(p, salt + k), seq=seq & 0xffffffff, ident=(ident + k) & 0xffff,
                           flags=flags, **kw))
        seq += p
    return out


def groups(frames, **kw):
    """The model's outputs of `frames` as lists of member payload lengths (a frame that is
    not TCP counts its length), with every merged output checked against the oracle."""
    hb = sm.pack(frames)
    recs = sm.oracle_records(hb)
    out, first, totals, mss = cm.coalesce(hb, recs, **kw)
    n = len(kw["order"]) if kw.get("order") is not None else hb.n
    assert int(totals[0]) == len(out) and int(totals[1]) == sum(len(o) for o in out)
    assert (first[len(out):] == n).all() and (mss[len(out):] == 0).all()
    check_outputs(out, mss)
    P = cm.positions(hb, recs, kw.get("order"), kw.get("trust_sums", False))
    return [[P[i].p for i in range(int(first[j]), int(first[j + 1]))] for j in range(len(out))]


def check_outputs(out, mss):
    """Every merged output re-parses through the oracle as OK with both sums valid."""
    hb = sm.pack(out)
    recs = sm.oracle_records(hb)
    merged = np.nonzero(mss[:len(out)])[0]
    v4 = cm.dispatch_ethertype(recs) == 0x0800
    for j in merged:
        r = recs[j]
        assert r["status"] == 0 and r["l4_sum"] == 0xffff, j
        assert r["ip_sum"] == (0xffff if v4[j] else 0), j
        assert int(r["payload_off"]) + int(r["payload_len"]) == len(out[j])
    return len(merged)


@pytest.mark.parametrize("mss", sm.MSS_VALUES)
def test_coalescing_undoes_segmentation(mss):
    """coalesce(segment(F)) == F for the hand-built segment frames: a segmented frame comes
    back cut at payload_off + payload_len (segmentation drops the Ethernet padding)."""
    hb = sm.pack(sm.hand_frames(mss), 3)
    recs = sm.oracle_records(hb)
    seg, first, _ = sm.segment(hb, recs, mss)
    v6 = cm.dispatch_ethertype(recs) == 0x86DD
    want = []
    for i, f in enumerate(sm.frames_of(hb)):
        cut = sm.is_segmented(recs[i], bool(v6[i]), mss)
        want.append(f[:int(recs[i]["payload_off"]) + int(recs[i]["payload_len"])] if cut else f)
    hs = sm.pack(seg)
    out, src_first, totals, out_mss = cm.coalesce(hs, sm.oracle_records(hs))
    assert out == want
    assert np.array_equal(src_first[:hb.n + 1], first)              # the inverse mapping
    n_seg = int((np.diff(first.astype(np.int64)) > 1).sum())
    assert check_outputs(out, out_mss) == n_seg == int((out_mss != 0).sum())
    assert (n_seg == 0) == (mss == 65535) and (mss == 65535 or n_seg >= 20)
    assert set(out_mss[out_mss != 0].tolist()) <= {mss}
    if mss in (536, 1448):                                          # the greedy tail rule
        assert len(out[-1]) == 14 + 65535 and int(np.diff(first.astype(np.int64))[-1]) == -(-65495 // mss)


def test_an_option_byte_or_the_window_breaks_a_link():
    a, b, c = stream([100, 100, 100], doff=8)
    assert groups([a, b, c]) == [[100, 100, 100]]
    assert groups([a, patched(b, 34 + 27, b"\x99"), c]) == [[100], [100], [100]]   # an option byte
    assert groups([a, b, patched(c, 34 + 31, b"\x99")]) == [[100, 100], [100]]
    assert groups([a, b, patched(c, 34 + 14, b"\x20\x01")]) == [[100, 100], [100]]
    assert groups([a, b, patched(c, 34 + 8, b"\x0a\x0b\x0c\x0e")]) == [[100, 100], [100]]     # ack


def test_seq_and_ident_must_run_on():
    a, b, c = stream([100, 100, 100])
    gap = sm.tcp4(sm.payload_bytes(100, 1), seq=1101, ident=8, flags=ACK)
    assert groups([a, gap, c]) == [[100], [100], [100]]
    skip = sm.tcp4(sm.payload_bytes(100, 1), seq=1100, ident=9, flags=ACK)          # ident + 2
    assert groups([a, skip]) == [[100], [100]]
    a, skip = (sm.tcp4(sm.payload_bytes(100, k), seq=1000 + 100 * k, ident=7 + 2 * k, flags=ACK,
                       frag=0x4000) for k in (0, 1))
    assert groups([a, skip]) == [[100, 100]]                                        # DF: ignored
    a, b = stream([100, 100], seq=0xffffffc0, ident=0xffff)                         # both wrap
    assert groups([a, b]) == [[100, 100]]


def test_flags():
    a, b, c, d = stream([100] * 4)
    psh = stream([100, 100], flags=ACK | PSH, salt=0)[1]
    assert psh[54:] == b[54:]
    assert groups([a, psh, c, d]) == [[100, 100], [100, 100]]                       # PSH ends a group
    out, _, _, _ = cm.coalesce(sm.pack([a, psh]), sm.oracle_records(sm.pack([a, psh])))
    assert out[0][47] == ACK | PSH                                                   # and is carried
    cwr = stream([100, 100, 100], flags=ACK | CWR)
    assert groups([a, cwr[1], c]) == [[100], [100, 100]]                            # CWR: a head only
    syn = stream([100, 100], flags=ACK | cm.SYN)[1]
    assert groups([a, syn, c]) == [[100], [100], [100]]
    fin = stream([100, 100], flags=ACK | FIN)[1]
    assert groups([a, fin, c]) == [[100, 100], [100]]


def test_shrinking_segments():
    assert groups(stream([1000, 500, 500, 500])) == [[1000, 500], [500, 500]]
    assert groups(stream([1000, 500, 300, 300])) == [[1000, 500], [300], [300]]
    assert groups(stream([500, 1000, 1000])) == [[500], [1000, 1000]]               # growing: a new head


def test_a_bad_tcp_sum_is_not_laundered():
    a, b, c = stream([100, 100, 100])
    bad = bytearray(b)
    bad[60] ^= 0x40
    assert groups([a, bytes(bad), c]) == [[100], [100], [100]]
    assert groups([a, bytes(bad), c], trust_sums=True) == [[100, 100, 100]]
    bad_ip = bytearray(b)
    bad_ip[24] ^= 1                                                                  # IPv4 checksum
    assert groups([a, bytes(bad_ip), c]) == [[100], [100], [100]]


def test_max_payload_cuts_a_run():
    s = stream([100] * 5)
    assert groups(s, max_payload=250) == [[100, 100], [100, 100], [100]]
    assert groups(s, max_payload=99) == [[100]] * 5
    assert groups(stream([100, 100, 100, 100, 40]), max_payload=240) == [[100, 100], [100, 100, 40]]
    assert groups(stream([100, 100, 100, 100, 50]), max_payload=240) == [[100, 100], [100, 100], [50]]


def test_two_packets_of_one_stream_merge_across_their_boundary():
    one = sm.tcp4(sm.payload_bytes(3000, 1), seq=5000, ident=20, flags=ACK)
    two = sm.tcp4(sm.payload_bytes(3000, 2), seq=8000, ident=23, flags=ACK | PSH)
    hb = sm.pack([one, two])
    seg, _, _ = sm.segment(hb, sm.oracle_records(hb), 1000)
    assert len(seg) == 6 and groups(seg) == [[1000] * 6]
    out, _, _, mss = cm.coalesce(sm.pack(seg), sm.oracle_records(sm.pack(seg)))
    assert out[0][54:] == one[54:] + two[54:] and out[0][47] == ACK | PSH and mss[0] == 1000


def test_an_order_entry_past_n_is_an_empty_frame():
    a, b = stream([100, 100])
    assert groups([a, b]) == [[100, 100]]
    hb = sm.pack([a, b])
    out, first, totals, mss = cm.coalesce(hb, sm.oracle_records(hb), order=[0, 2, 1, 0xffffffff])
    assert out == [a, b"", b, b""] and first.tolist() == [0, 1, 2, 3, 4] and not mss.any()


def with_port(f, port):
    return patched(f, 34, port.to_bytes(2, "big"))


def test_flow_order_brings_interleaved_streams_together():
    streams = [[with_port(f, 5000 + 7 * s) for f in stream([200] * 6, seq=999 * s, ident=50 * s, salt=s)]
               for s in range(3)]
    mixed = [streams[k % 3][k // 3] for k in range(18)]                             # round robin
    hb = sm.pack(mixed)
    assert groups(mixed) == [[200]] * 18                                             # nothing merges
    order = cm.flow_order_host(hb)
    assert order.dtype == np.uint32 and sorted(order.tolist()) == list(range(18))
    assert sorted(groups(mixed, order=order)) == [[200] * 6] * 3
    out, first, _, _ = cm.coalesce(hb, sm.oracle_records(hb), order=order)
    assert sorted(o[54:] for o in out) == sorted(b"".join(f[54:] for f in s) for s in streams)


def test_the_exports_and_wrappers_exist():
    assert {"rpkt_gpu_coalesce_batch", "rpkt_gpu_coalesce_workspace_bytes"} <= set(engine.EXPORTS)
    assert callable(engine.coalesce_batch) and callable(engine.coalesce_workspace)
    assert callable(engine.flow_order) and engine.COALESCE_TRUST_SUMS == 1
    from rpkt_amd.build import build_gpu
    build_gpu()
    ws = engine.lib().rpkt_gpu_coalesce_workspace_bytes
    assert ws(1) >= 44 and ws(70000) >= 70000 * 44 and ws(70000) % 16 == 0
