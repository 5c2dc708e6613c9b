"""tests/segment_chains_model.py on the CPU: the flattening under rpkt_chains_t's clamps, the
chain builder, and that tests/segment_model.py takes oracle.parse_chains' records as it is
(their offsets are logical positions in the chain's bytes)."""
import numpy as np

from oracle import oracle
from rpkt_amd import gen

import segment_chains_model as scm
import segment_model as sm


def test_single_segment_chains_give_the_flat_models_output():
    for mss in (7, 17, 536):
        frames = sm.hand_frames(mss)
        hb = sm.pack(frames)
        hc = scm.chains_of(frames, [[] for _ in frames], lead=3)
        assert scm.chain_bytes(hc) == frames
        want = sm.segment(hb, sm.oracle_records(hb), mss)
        # one segment per chain: the chain parse sees what the flat parse sees
        recs = scm.chain_records(hc)
        assert recs.tobytes() == sm.oracle_records(hb).tobytes()
        got = scm.segment_chains(hc, recs, mss)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_builder_places_segments_shuffled_at_odd_gaps_with_empty_ones():
    frames = [sm.tcp4(sm.payload_bytes(100, k)) for k in range(6)]
    cuts = [[0, 10], [54, 54], [20, 60, 100], [], [154], [1, 2, 3]]
    hc = scm.chains_of(frames, cuts, lead=5)
    assert scm.chain_bytes(hc) == frames and [hc.frame(p) for p in range(6)] == frames
    assert hc.chain_first.tolist() == [0, 3, 6, 10, 11, 13, 17]
    lens = hc.segs[:, 1].tolist()
    assert lens[0] == 0 and lens[4] == 0 and lens[12] == 0      # first, middle, last empty
    starts = hc.segs[:, 0].astype(np.int64)
    assert (np.diff(starts) < 0).any()                          # not in chain order
    assert len(set((starts % 16).tolist())) > 4                 # many byte phases
    order = np.argsort(starts, kind="stable")
    gaps = starts[order][1:] - (starts[order] + hc.segs[order, 1])[:-1]
    assert (gaps % 2 == 1).all()


def test_tso_tx_frame_at_every_two_segment_cut():
    """The reference's 4054-byte super-frame cut anywhere into two segments: four wire frames
    of 1024, 1024, 1024 and 928 payload bytes whatever the cut, with the flattened bytes'
    records; with the chain parse's records, a cut inside the headers passes through."""
    f = sm.tso_tx_frame()
    flat = sm.segment(sm.pack([f]), sm.oracle_records(sm.pack([f]), 3), 1024)
    assert flat[2].tolist() == [4, 4000 + 4 * 54]
    cuts = list(range(len(f) + 1))
    hc = scm.chains_of([f] * len(cuts), [[c] for c in cuts], lead=1)
    out, first, totals = scm.segment_chains(hc, scm.flat_records(hc, 3), 1024)
    assert np.array_equal(first, 4 * np.arange(len(cuts) + 1))
    assert totals.tolist() == [4 * len(cuts), len(cuts) * (4000 + 4 * 54)]
    assert out == flat[0] * len(cuts)
    # Pbuf rules: a header is tested against the segment that holds its first byte, so it may
    # start where a segment ends (c = 14, 34) but not straddle an end; Pbuf::new starts at
    # segment 0 even when it is empty (c = 0)
    recs = scm.chain_records(hc, 3)
    _, first, _ = scm.segment_chains(hc, recs, 1024)
    n_out = np.diff(first.astype(np.int64))
    whole = [14, 34] + list(range(54, len(cuts)))
    assert np.nonzero(n_out == 4)[0].tolist() == whole and set(n_out.tolist()) == {1, 4}
    assert np.nonzero(recs["status"] == 0)[0].tolist() == whole


def test_model_composes_with_parse_chains_records():
    """Config 7 in the mbuf layout (8000-byte frames in 2048-byte rooms, half of them TCP):
    the chain parse's records are the flat parse's there, offsets and all, so the model needs
    no translation; in a fuzz layout the two differ only where a header straddles a cut."""
    hc = gen.make_chains(7, 512, layout="mbuf")
    recs = scm.chain_records(hc)
    flat = scm.flat_records(hc)
    assert recs.tobytes() == flat.tobytes()
    out, first, totals = scm.segment_chains(hc, recs, 1448)
    share = (np.diff(first.astype(np.int64)) > 1).mean()
    assert abs(share - 0.498) < 0.001, share
    assert int(totals[0]) == len(out) and int(totals[1]) == sum(len(o) for o in out)
    # every payload byte is carried exactly once
    for p in np.nonzero(np.diff(first.astype(np.int64)) > 1)[0][:20]:
        f, r = hc.frame(p), recs[p]
        po, pl = int(r["payload_off"]), int(r["payload_len"])
        parts = out[int(first[p]):int(first[p + 1])]
        assert b"".join(x[po:] for x in parts) == f[po:po + pl]
    hz = gen.make_chains(5, 2048, layout="fuzz")
    rz, fz = scm.chain_records(hz), scm.flat_records(hz)
    differ = np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(rz, fz)])[0]
    assert 0 < len(differ) < hz.n and (rz["status"][differ] != 0).all()


def test_clamps_of_out_of_range_descriptors():
    """chain_first entries past n_segs and decreasing, segment offsets and lengths past the
    arena: the documented clamps, nothing else."""
    frames = [sm.tcp4(sm.payload_bytes(40, k)) for k in range(4)]
    hc = scm.chains_of(frames, [[30], [], [10, 20], [50]], shuffle=False)
    assert hc.chain_first.tolist() == [0, 2, 3, 6, 8]
    fb = hc.buf.size
    # chain 0: [0, 2); chain 1: a = 2, b = max(1, 2) = 2: empty; chain 2: [1, 6);
    # chain 3: a = min(6, 8), b = min(1000, 8); chain 4: a = 8 = n_segs: empty
    hc.chain_first = np.array([0, 2, 1, 6, 1000, 7], dtype=np.uint32)
    hc.n = 5
    segs = hc.segs.copy()
    segs[7] = (segs[7][0], 0xffffffff)                          # length past the arena
    segs[6] = (fb + 5, 7)                                       # offset past the arena
    hc.segs = segs
    got = scm.chain_bytes(hc)
    assert got[0] == frames[0] and got[1] == b"" and got[4] == b""
    assert got[2] == frames[0][30:] + frames[1] + frames[2]
    assert got[3] == hc.buf[int(segs[7][0]):].tobytes()
    hb = scm.flatten(hc)
    assert hb.n == 5 and sm.frames_of(hb) == got
    # the oracle's chain parse clamps the same way: frame_len is the clamped pkt_len
    recs = oracle.parse_chains(hc.buf, hc.segs, hc.chain_first, sm.F6)
    assert recs["frame_len"].tolist() == [len(g) for g in got]
