"""tests/nested_tunnel_ref.py (the reference of rpkt_gpu_parse_tunnel_next, a composition of
oracle.tunnel_batch) against answers worked out by hand from the header sizes, its own
self-check on the nested fuzz set, the coverage that set gives, and a walk of both levels
with the host views (rpkt_amd/tunviews.py)."""
import numpy as np

from rpkt_amd.records import F_IPV6, STATUS, TUN_KIND, TUN_STATUS
from rpkt_amd.tunviews import Gre, Gtpv1, TunnelPacket, Vxlan
from rpkt_amd.views import EtherFrame, Ipv4, Ipv6, Udp

import nested_tunnel_ref as ref

F6 = 3 | F_IPV6


def test_hand_built_frames():
    """Offsets by header sizes.  GTP-U in VXLAN: 14 + 20 + 8 + 8 (VXLAN) = 50, the inner
    Ethernet frame; + 14 + 20 + 8 = 92, the GTP header; + 8 = 100.  VXLAN in GRE with
    checksum: 14 + 20 + 8 (GRE) = 42, the inner IP packet; + 20 + 8 = 70; + 8 = 78.  GRE with
    a key in GTP-U over IPv6: 14 + 40 + 8 + 8 (GTP) = 70, the inner IPv6 packet; + 40 = 110;
    + 8 = 118."""
    hb = ref.pack(ref.hand_frames())
    o, t, i = ref.level1(hb, F6)
    assert list(t["kind"]) == [TUN_KIND["VXLAN"], TUN_KIND["GRE"], TUN_KIND["GTPU"]]
    assert list(t["inner_off"]) == [50, 42, 70] and (t["status"] == TUN_STATUS["OK"]).all()
    t2, i2 = ref.next_level(hb, F6, t, i)
    assert list(t2["kind"]) == [TUN_KIND["GTPU"], TUN_KIND["VXLAN"], TUN_KIND["GRE"]]
    assert (t2["status"] == TUN_STATUS["OK"]).all()
    assert list(t2["tun_off"]) == [92, 70, 110] and list(t2["inner_off"]) == [100, 78, 118]
    assert int(t2["id"][0]) == 0xdeadbeef and int(t2["id"][1]) == 0x123456 and int(t2["id"][2]) == 0x1234
    assert (i2["status"] == STATUS["OK"]).all() and (i2["l4_sum"] == 0xffff).all()
    assert (i2["ip_sum"] == 0xffff).all()
    # the innermost packets: inner_udp4(40) = 20 + 8 + 40 bytes (behind an Ethernet header
    # in the second frame), offsets in the outermost frame
    assert list(i2["frame_len"]) == [68, 82, 68]
    assert list(i2["l3_off"]) == [100, 92, 118] and list(i2["payload_off"]) == [128, 120, 146]
    assert list(i2["ethertype"]) == [0x0800, 0x0800, 0x0800] and (i2["n_vlan"] == 0).all()

    # without RPKT_F_IPV6 the third frame's outer IPv6 header is not parsed: no level 1
    o, t, i = ref.level1(hb, 3)
    assert int(t["kind"][2]) == TUN_KIND["NONE"]
    t2, i2 = ref.next_level(hb, 3, t, i)
    assert list(t2["status"]) == [TUN_STATUS["OK"], TUN_STATUS["OK"], TUN_STATUS["NONE"]]
    assert int(t2["kind"][2]) == TUN_KIND["NONE"] and int(i2["status"][2]) == STATUS["NO_INNER"]
    assert i2[2].tobytes()[1:] == bytes(79) and t2[2].tobytes()[2:] == bytes(14)


def test_three_levels():
    hb = ref.pack(ref.three_level_frames())
    o, t, i = ref.level1(hb, F6)
    t2, i2 = ref.next_level(hb, F6, t, i)
    t3, i3 = ref.next_level(hb, F6, t2, i2)
    for lv, kind in ((t, "GTPU"), (t2, "GRE"), (t3, "VXLAN")):
        assert (lv["kind"] == TUN_KIND[kind]).all() and (lv["status"] == TUN_STATUS["OK"]).all()
    # 14 + 20 + 8 + 12 (GTP with sequence) = 54; + 20 = 74 (GRE), + 4 = 78; + 20 + 8 = 106, + 8
    assert (int(t["inner_off"][0]), int(t2["tun_off"][0]), int(t2["inner_off"][0]),
            int(t3["tun_off"][0]), int(t3["inner_off"][0])) == (54, 74, 78, 106, 114)
    assert (i3["status"] == STATUS["OK"]).all() and (i3["l4_sum"] == 0xffff).all()
    t4, i4 = ref.next_level(hb, F6, t3, i3)                    # nothing deeper
    assert (t4["status"] == TUN_STATUS["NONE"]).all() and (i4["status"] == STATUS["NO_INNER"]).all()


def test_self_check_and_coverage_of_the_nested_fuzz_set():
    """next_level asserts that the sub-frame's outer record is the level-1 inner record.  With
    RPKT_F_IPV6 (two of the six wrappings have IPv6 outers) more than 40 % of the frames
    decode a second tunnel (53 % here); every second-level tunnel status and at least 8
    innermost statuses occur."""
    for flags in (F6, 3):
        hb = ref.nested_frames(14, 2048, seed=14)
        o, t, i = ref.level1(hb, flags)
        t2, i2 = ref.next_level(hb, flags, t, i)
        assert set(np.unique(t2["status"])) == set(TUN_STATUS.values())
        assert len(np.unique(i2["status"])) >= 8
        if flags == F6:
            assert (t2["status"] == TUN_STATUS["OK"]).mean() >= 0.40
        # a frame without a level-1 inner frame has no level 2
        none = t["status"] != TUN_STATUS["OK"]
        assert (t2["status"][none] == TUN_STATUS["NONE"]).all()
        assert (i2["status"][none] == STATUS["NO_INNER"]).all()
    hb13 = ref.nested_frames(13, 300, seed=13)
    o, t, i = ref.level1(hb13, F6)
    t2, i2 = ref.next_level(hb13, F6, t, i)
    assert (t2["status"] == TUN_STATUS["OK"]).mean() > 0.8


def test_expected_events_replace_only_decoded_second_tunnels():
    from oracle import oracle
    hb = ref.nested_frames(14, 600, seed=3)
    o, t, i = ref.level1(hb, F6)
    ev1 = oracle.tunnel_flow_events(o, t, i, 97)
    t2, i2, sub = ref.next_level(hb, F6, t, i, with_sub=True)
    ev2 = ref.expected_events(ev1, sub, 97)
    ok = t2["status"] == TUN_STATUS["OK"]
    assert np.array_equal(ev2[~ok], ev1[~ok]) and (ev2[ok] != ev1[ok]).any()
    assert np.array_equal(ev2[ok] & np.uint64(0xffffffff), i2["frame_len"][ok].astype(np.uint64))


def test_views_walk_both_levels():
    """Vxlan.parse(udp.payload()) -> EtherFrame.parse -> ... -> Gtpv1.parse(udp.payload()):
    the first hand-built frame read through both levels, as one chain (the next level's
    records travel with the payload cursor) and started again at the level-1 inner frame."""
    frames = ref.hand_frames()
    hb = ref.pack(frames)
    o, t, i = ref.level1(hb, F6)
    t2, i2 = ref.next_level(hb, F6, t, i)
    pkt = TunnelPacket(o[0], t[0], i[0], frames[0], deeper=[(t2[0], i2[0])])
    udp = Udp.parse(Ipv4.parse(EtherFrame.parse(pkt).unwrap().payload()).unwrap().payload()).unwrap()
    vx = Vxlan.parse(udp.payload()).unwrap()
    assert vx.vni() == 0x123456
    eth = EtherFrame.parse(vx.payload()).unwrap()
    udp2 = Udp.parse(Ipv4.parse(eth.payload()).unwrap().payload()).unwrap()
    assert udp2.dst_port() == 2152 and udp2.payload().cursor() == 92
    gtp = Gtpv1.parse(udp2.payload()).unwrap()
    assert gtp.teid() == 0xdeadbeef and gtp.message_type() == 255 and gtp.packet_len() == 76
    ip = Ipv4.parse(gtp.t_pdu()).unwrap()
    assert ip.buf.cursor() == 100 and ip.verify_checksum() and ip.src_addr() == "192.168.0.1"
    u3 = Udp.parse(ip.payload()).unwrap()
    assert u3.dst_port() == 53 and u3.sum() == 0xffff and u3.payload().cursor() == 128
    # the second level alone, from the level-1 inner record
    p2 = TunnelPacket(i[0], t2[0], i2[0], frames[0])
    udp2 = Udp.parse(Ipv4.parse(EtherFrame.parse(p2).unwrap().payload()).unwrap().payload()).unwrap()
    assert Gtpv1.parse(udp2.payload()).unwrap().teid() == 0xdeadbeef
    # a level-1 inner IP packet: the chain starts at its IP header (parent = the level-1 tunnel)
    p3 = TunnelPacket(i[2], t2[2], i2[2], frames[2], parent=t[2])
    ip6 = Ipv6.parse(p3).unwrap()
    assert p3.cursor() == 70 and ip6.next_header() == 47
    gre = Gre.parse(ip6.payload()).unwrap()
    assert gre.key() == 0x1234 and Ipv4.parse(gre.payload()).unwrap().buf.cursor() == 118
    # one level of records walks as before
    p1 = TunnelPacket(o[0], t[0], i[0], frames[0])
    udp = Udp.parse(Ipv4.parse(EtherFrame.parse(p1).unwrap().payload()).unwrap().payload()).unwrap()
    eth = EtherFrame.parse(Vxlan.parse(udp.payload()).unwrap().payload()).unwrap()
    udp2 = Udp.parse(Ipv4.parse(eth.payload()).unwrap().payload()).unwrap()
    assert Gtpv1.parse(udp2.payload()).is_err()                 # no second-level records given
