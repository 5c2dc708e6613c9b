"""The reference of rpkt_gpu_parse_tunnel_next for the tests: a composition of the frozen
oracle (oracle.tunnel_batch), no second decode.

The level-k inner frame of frame i is bytes [inner_off, inner_off + inner.frame_len) of it.
Handed to oracle.tunnel_batch as a frame of its own -- as it is when it is an Ethernet frame
(inner_type 0x6558), behind a synthetic 14-byte Ethernet header (MACs 0, ethertype =
inner_type) when it is an IP packet -- its OUTER record is the level-k inner record again
(next_level asserts that), and its tunnel and inner records are level k + 1, once every
offset is moved from the sub-frame back into the outermost frame.  The oracle's own rebasing
leaves exactly the offsets it never reached at zero, so "add the shift where nonzero" is
exact.  Shared by the CPU test of this helper and the GPU tests of the entry."""
import struct

import numpy as np

from oracle import oracle
from rpkt_amd import gen
from rpkt_amd.records import REC_DTYPE, STATUS, TUN_DTYPE, TUN_KIND, TUN_STATUS, is_ip6

import tunnel_frames as tf

REC_OFFS = ("l3_off", "l4_off", "payload_off")


def pack(frames, lead=0):
    """Packed HostBatch of a list of byte strings; a `lead`-byte junk frame first shifts
    every following frame's alignment (16 spare bytes at the end)."""
    parts = ([b"\xee" * lead] if lead else []) + [bytes(f) for f in frames]
    offs = np.zeros(len(parts) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(p) for p in parts])
    blob = np.frombuffer(b"".join(parts) + bytes(16), dtype=np.uint8).copy()
    return gen.HostBatch(0, len(parts), 0, blob, offs, 0, 0)


def frames_of(hb):
    """The frames of a HostBatch (packed or strided) as byte strings."""
    if hb.offsets is not None:
        return [hb.frames[int(hb.offsets[i]):int(hb.offsets[i + 1])].tobytes() for i in range(hb.n)]
    flen = hb.frame_len or hb.stride
    return [hb.frames[i * hb.stride:i * hb.stride + flen].tobytes() for i in range(hb.n)]


def level1(hb, flags):
    return oracle.tunnel_batch(hb.frames, hb.n, flags, offsets=hb.offsets, stride=hb.stride,
                               frame_len=hb.frame_len)


def rebase_records(recs, shift):
    """recs with `shift` added to every offset field that is nonzero (ip6_pdst_off, record
    bytes 34..35, on IPv6 records)."""
    out = recs.copy()
    shift = np.asarray(shift, dtype=np.int64)
    for f in REC_OFFS:
        v = out[f].astype(np.int64)
        out[f] = np.where(v != 0, v + shift, 0).astype(np.uint16)
    raw = out.view(np.uint8).reshape(-1, 80)
    pd = raw[:, 34].astype(np.int64) | (raw[:, 35].astype(np.int64) << 8)
    new = np.where(is_ip6(recs) & (pd != 0), pd + shift, pd)
    raw[:, 34] = new & 0xff
    raw[:, 35] = (new >> 8) & 0xff
    return out


def rebase_tunnels(tun, shift):
    out = tun.copy()
    shift = np.asarray(shift, dtype=np.int64)
    for f in ("tun_off", "inner_off"):
        v = out[f].astype(np.int64)
        out[f] = np.where(v != 0, v + shift, 0).astype(np.uint16)
    return out


def next_level(hb, flags, tun, inner, with_sub=False):
    """The expected (tun_next, inner_next) of rpkt_gpu_parse_tunnel_next on batch `hb` with
    the level-k records (tun, inner).  with_sub: also (idx, o', t', i'), the oracle's
    un-rebased records of the sub-frames of the frames idx (for the expected events)."""
    frames = frames_of(hb)
    tun_next = np.zeros(hb.n, dtype=TUN_DTYPE)
    tun_next["kind"] = TUN_KIND["NONE"]
    tun_next["status"] = TUN_STATUS["NONE"]
    inner_next = np.zeros(hb.n, dtype=REC_DTYPE)
    inner_next["status"] = STATUS["NO_INNER"]
    idx = np.nonzero(tun["status"] == TUN_STATUS["OK"])[0]
    subs, shift, synth = [], [], []
    for i in idx:
        off, n = int(tun["inner_off"][i]), int(inner["frame_len"][i])
        sub = frames[i][off:off + n]
        assert len(sub) == n, "level-k inner frame inside frame %d" % i
        if int(tun["inner_type"][i]) == 0x6558:
            subs.append(sub)
            shift.append(off)
            synth.append(0)
        else:
            subs.append(bytes(12) + struct.pack("!H", int(tun["inner_type"][i])) + sub)
            shift.append(off - 14)
            synth.append(14)
    empty = (np.zeros(0, REC_DTYPE), np.zeros(0, TUN_DTYPE), np.zeros(0, REC_DTYPE))
    if len(idx) == 0:
        return (tun_next, inner_next, (idx,) + empty) if with_sub else (tun_next, inner_next)
    sb = pack(subs)
    o2, t2, i2 = oracle.tunnel_batch(sb.frames, sb.n, flags, offsets=sb.offsets)
    shift = np.array(shift, dtype=np.int64)
    # the helper's self-check: the sub-frame's outer record is the level-k inner record
    chk = rebase_records(o2, shift)
    chk["frame_len"] -= np.array(synth, dtype=np.uint32)
    if chk.tobytes() != inner[idx].tobytes():
        k = int(np.nonzero(chk != inner[idx])[0][0])
        raise AssertionError("sub-frame %d (frame %d): outer record %s is not the level-k inner "
                             "record %s" % (k, idx[k], chk[k], inner[idx][k]))
    tun_next[idx] = rebase_tunnels(t2, shift)
    inner_next[idx] = rebase_records(i2, shift)
    return (tun_next, inner_next, (idx, o2, t2, i2)) if with_sub else (tun_next, inner_next)


def expected_events(ev_before, sub, n_buckets):
    """The events after the next-level call: `ev_before` (the level before's), replaced by
    the innermost record's event where the next tunnel decoded."""
    idx, o2, t2, i2 = sub
    ev = np.array(ev_before, dtype=np.uint64, copy=True)
    if len(idx):
        e2 = oracle.tunnel_flow_events(o2, t2, i2, n_buckets)
        ok = t2["status"] == TUN_STATUS["OK"]
        ev[idx[ok]] = e2[ok]
    return ev


def wrap(k, f):
    """Frame f (an Ethernet frame) inside a second tunnel, by k % 6."""
    m = k % 6
    if m == 0:
        return tf.ether(0x0800, tf.ipv4_packet(17, tf.udp(40000, 4789, tf.vxlan(f))))
    if m == 1:
        return tf.ether(0x86dd, tf.ipv6_packet(17, tf.udp(4789, 4789, tf.vxlan(f))))
    if m == 2:
        return tf.ether(0x0800, tf.ipv4_packet(47, tf.gre(f, proto=0x6558, checksum=True)))
    if m == 3:
        return tf.ether(0x0800, tf.ipv4_packet(17, tf.udp(2152, 2152, tf.gtpu(f[14:]))))
    if m == 4:
        return tf.ether(0x86dd, tf.ipv6_packet(47, tf.gre(f[14:], proto=0x0800, key=k)))
    return f


def nested_frames(cfg, n, seed, lead=0):
    """Two-level tunnel frames: the generator's tunnel frames (config 13 or 14), frame k
    wrapped by k % 6 (5: left as it is, a single-level frame in the same tile), packed."""
    return pack([wrap(k, f) for k, f in enumerate(frames_of(gen.make_batch(cfg, n, seed=seed)))],
                lead)


# ---- the hand-built frames ------------------------------------------------------

def hand_parts(payload=40):
    """The three hand-built frames as (level-1 wrapping, mid-level wrapping, second tunnel
    header, innermost frame), so a test can cut the innermost bytes and still have
    well-formed levels around them."""
    inner = tf.inner_udp4(payload)
    return [
        (lambda m: tf.ether(0x0800, tf.ipv4_packet(17, tf.udp(40000, 4789, tf.vxlan(m)))),
         lambda x: tf.ether(0x0800, tf.ipv4_packet(17, tf.udp(2152, 2152, x))),
         tf.gtpu, inner),
        (lambda m: tf.ether(0x0800, tf.ipv4_packet(47, tf.gre(m, checksum=True))),
         lambda x: tf.ipv4_packet(17, tf.udp(40001, 4789, x)),
         tf.vxlan, tf.ether(0x0800, inner)),
        (lambda m: tf.ether(0x86dd, tf.ipv6_packet(17, tf.udp(2152, 2152, tf.gtpu(m)))),
         lambda x: tf.ipv6_packet(47, x),
         lambda p: tf.gre(p, key=0x1234), inner)]


def hand_frames(payload=40):
    """[GTP-U in VXLAN (IPv4 outers, 8-B GTP header), VXLAN in GRE-with-checksum over IPv4,
    GRE (key) in GTP-U over IPv6 outers], each around inner_udp4(payload)."""
    return [w(m(t(p))) for w, m, t, p in hand_parts(payload)]


def hand_cuts(payload=40):
    """The hand-built frames cut at every byte, three ways: the innermost frame cut (inside
    its IP / L4 headers and its payload) with every header around it made for the cut bytes;
    the second tunnel's header and payload cut (inside the tunnel header too) with the
    mid-level headers made for them; the level-1 inner frame itself cut (a mid level that no
    longer parses)."""
    out = []
    for w, m, t, p in hand_parts(payload):
        x = t(p)
        out += [w(m(t(p[:c]))) for c in range(len(p) + 1)]
        out += [w(m(x[:c])) for c in range(len(x) + 1)]
        out += [w(m(x)[:c]) for c in range(len(m(x)) + 1)]
    return out


def deep_frame(payload):
    """A second tunnel that starts past the outer 128-B header window: an IPv6 outer with
    three extension headers and a GTP-U chain of three extension headers (level-1 inner
    packet at byte 166) around a VXLAN frame with `payload` innermost UDP bytes."""
    t = tf.ipv4_packet(17, tf.udp(40000, 4789, tf.vxlan(tf.ether(0x0800, tf.inner_udp4(payload)))))
    exts = [(0x81, bytes(range(30)))] * 2 + [(0x85, bytes([0x10, 1]))]
    u = tf.ipv6_packet(17, tf.udp(2152, 2152, tf.gtpu(t, exts, seq=77)))[40:]   # checksum filled
    ext = b"".join(bytes([nh, 0, 1, 4, 0, 0, 0, 0]) for nh in (60, 60, 17))     # hbh, dst, dst
    ip6 = tf.ipv6_packet(0, ext + u)
    return tf.ether(0x86dd, ip6)


def three_level_frames(payload=40):
    """VXLAN in GRE in GTP-U (and a second with an Ethernet GRE payload and a longer
    innermost packet): level 1 GTP-U, level 2 GRE, level 3 VXLAN."""
    out = []
    for p, key in ((payload, None), (payload + 301, 5)):
        vx = tf.ipv4_packet(17, tf.udp(40002, 4789, tf.vxlan(tf.ether(0x0800, tf.inner_udp4(p)))))
        g = tf.ipv4_packet(47, tf.gre(vx, key=key))
        out.append(tf.ether(0x0800, tf.ipv4_packet(17, tf.udp(2152, 2152, tf.gtpu(g, seq=9)))))
    vx = tf.ether(0x0800, tf.ipv4_packet(17, tf.udp(4789, 4789, tf.vxlan(
        tf.ether(0x0800, tf.inner_udp4(payload + 7))))))
    g = tf.ipv6_packet(47, tf.gre(vx, proto=0x6558, checksum=True))
    out.append(tf.ether(0x86dd, tf.ipv6_packet(17, tf.udp(2152, 2152, tf.gtpu(g)))))
    return out
