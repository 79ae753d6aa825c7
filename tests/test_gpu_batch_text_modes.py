"""Every route by which a finished batch becomes text (Engine.run_batches: device_text, multiple_files, device_gzip,
device_gzip_clusters, defer_patterns, targets_sink, cluster_targets_sink) reduced to plain bytes and compared with the
host renderers' bytes of the same engine options; the counters a batch reports about its text; and a batch that falls
back to the host renderers in the middle of a device-text run that has a sink."""
import gzip

import pytest

pytestmark = pytest.mark.gpu

K = 21
TEXT_TILE = 24576               # bytes of text one workgroup of the text kernels lays out


def kh_refused(name_len, k=K):
    """whether the kmers_to_hashes text kernel refuses a cluster name of this length: a cluster's head and one row must
    fit one tile -- kh_head_len(L) + kh_row_len(L, k) > TEXT_TILE, which is 2 L + k + 54 > 24576"""
    return 2 * name_len + k + 54 > TEXT_TILE


LAST_ON_DEVICE = (TEXT_TILE - K - 54) // 2      # 12250 at k = 21
assert not kh_refused(LAST_ON_DEVICE) and kh_refused(LAST_ON_DEVICE + 1) and LAST_ON_DEVICE == 12250


@pytest.fixture(scope="module")
def batch_input():
    from panfeed_amd import synth
    cl = synth.generate(6, 12, first=1723, mean_len=300, min_len=80, max_len=600, n_rate=0.2, paralog_rate=0.05)
    names = cl[0].names
    return {"recs": [c.record() for c in cl], "targets": set(names[::2]), "host": {}}


def _plain(data):
    """`data` of a BatchOutput or a sink -- str, bytes-like, GzipMembers -- as the bytes of text it stands for"""
    from panfeed_amd.engine import GzipMembers
    if isinstance(data, GzipMembers):
        text = gzip.decompress(bytes(data.view))
        assert data.text_bytes is None or data.text_bytes == len(text)
        return text
    return data.encode() if isinstance(data, str) else bytes(data)


class Reduced:
    """One run_stream run as plain bytes.  kt / kh / hp: kmers.tsv (the sink's blocks and every out.kmers_tsv, in the
    order they were produced), kmers_to_hashes, hashes_to_patterns; clusters: under multiple_files (idx, kt, kh, hp) per
    cluster, from per_cluster and the cluster sink; batches: per batch its stats, the types of its two bodies, the
    kmers.tsv bytes it produced, the text bytes its sink saw and the member bytes it handed out."""

    def __init__(self, recs, targets, batch_clusters=2, sink=None, defer_patterns=False, device_text=True, **engine_kw):
        from panfeed_amd.engine import Engine, GzipMembers
        eng = Engine(klength=K, max_strains=32, stroi=targets, **engine_kw)
        self.device_gzip = eng.device_gzip or eng.device_gzip_clusters
        produced, calls = [], []        # kmers.tsv pieces of the batch under way; the cluster sink's (idx, text)
        seen = {"text": 0, "members": 0, "kinds": []}

        def note(block):
            seen["kinds"].append(type(block))
            seen["members"] += len(block) if isinstance(block, GzipMembers) else 0
            text = _plain(block)
            seen["text"] += len(text)
            return text

        kw = {}
        if sink == "targets":
            kw["targets_sink"] = lambda block: produced.append(note(block))
        elif sink == "clusters":
            kw["cluster_targets_sink"] = lambda idx, block: calls.append((idx, note(block)))
        self.kt, self.kh, self.hp, self.clusters, self.batches = b"", b"", b"", [], []
        try:
            for out in eng.run_stream(recs, batch_clusters=batch_clusters, device_text=device_text,
                                      defer_patterns=defer_patterns, **kw):
                produced.append(_plain(out.kmers_tsv))
                handed = seen["members"]
                for body in (out.kmers_to_hashes, out.hashes_to_patterns):
                    handed += len(body) if isinstance(body, GzipMembers) else 0
                self.batches.append({"stats": dict(out.stats), "kt": b"".join(produced), "sink_text": seen["text"],
                                     "members": handed, "sink_kinds": seen["kinds"],
                                     "bodies": (type(out.kmers_to_hashes), type(out.hashes_to_patterns))})
                self.kt += b"".join(produced)
                self.kh += _plain(out.kmers_to_hashes)
                self.hp += _plain(out.hashes_to_patterns)
                if eng.multiple_files:
                    assert [c[0] for c in out.per_cluster] == [r[1] for r in recs[len(self.clusters):][:len(out.per_cluster)]]
                    if sink == "clusters":
                        # at least one call per cluster, in order, clusters without target rows included
                        order = [idx for i, (idx, _t) in enumerate(calls) if i == 0 or calls[i - 1][0] != idx]
                        assert order == [c[0] for c in out.per_cluster]
                    for idx, kt, kh, hp in out.per_cluster:
                        assert (kt is None) == (sink == "clusters")
                        kt = b"".join(t for i, t in calls if i == idx) if kt is None else _plain(kt)
                        self.clusters.append((idx, kt, _plain(kh), _plain(hp)))
                del produced[:], calls[:]
                seen.update(text=0, members=0, kinds=[])
        finally:
            eng.close()

    def texts(self):
        return self.kt, self.kh, self.hp, self.clusters

    def check_stats(self, device_text=True, multiple_files=False):
        assert len(self.batches) == 3
        for b in self.batches:
            st = b["stats"]
            if multiple_files:
                assert st["device_cluster_files"] == (st["clusters"] if device_text else 0)
            else:
                assert "device_cluster_files" not in st
            # members leave the device only: a device-text batch counts them exactly when a device gzip switch is on
            assert ("compressed_bytes" in st) == (device_text and self.device_gzip)
            assert st.get("compressed_bytes", 0) == b["members"]
        assert sum(b["stats"].get("kmers_tsv_streamed", 0) for b in self.batches) == sum(b["sink_text"] for b in self.batches)


def _host(batch_input, **engine_kw):
    """the host renderers' run of these engine options (made once, left unchanged)"""
    key = tuple(sorted(engine_kw.items()))
    if key not in batch_input["host"]:
        run = Reduced(batch_input["recs"], batch_input["targets"], device_text=False, **engine_kw)
        run.check_stats(device_text=False, multiple_files=bool(engine_kw.get("multiple_files")))
        batch_input["host"][key] = run
    return batch_input["host"][key]


def _smallest_budget(recs, targets, batch_clusters=2):
    """the smallest targets_text_budget every batch of the run accepts"""
    import seam_batch
    from panfeed_amd.engine import Engine
    from panfeed_amd.packing import build_batch_native
    eng = Engine(klength=K, max_strains=32, stroi=targets)
    try:
        need = []
        for at in range(0, len(recs), batch_clusters):
            hb = build_batch_native(recs[at:at + batch_clusters], K, True, eng.W, stroi=eng.stroi, first_ordinal=at)
            eng.submit_host_batch(hb)
            need.append(seam_batch.smallest_budget(eng, hb))
    finally:
        eng.close()
    return max(need)


# ---------------------------------------------------------------------------------------------- one pair of files
@pytest.mark.parametrize("sink,engine_kw", [(None, {}), ("targets", {}), ("targets", {"device_gzip": True})],
                         ids=["no_sink", "targets_sink", "device_gzip_targets_sink"])
def test_single_pair(batch_input, sink, engine_kw):
    host = _host(batch_input, **engine_kw)
    assert host.kt and host.kh and host.hp and not host.clusters
    run = Reduced(batch_input["recs"], batch_input["targets"], sink=sink, **engine_kw)
    assert run.texts() == host.texts()
    run.check_stats()
    for b in run.batches:
        assert b["stats"]["kmers_tsv_streamed"] == (len(b["kt"]) if sink else 0)
        assert str not in b["bodies"]


def test_single_pair_small_budget(batch_input):
    host = _host(batch_input)
    budget = _smallest_budget(batch_input["recs"], batch_input["targets"])
    run = Reduced(batch_input["recs"], batch_input["targets"], sink="targets", targets_text_budget=budget)
    assert run.texts() == host.texts()
    run.check_stats()
    assert max(b["stats"]["kmers_tsv_ranges"] for b in run.batches) > 1
    assert all(0 < b["stats"]["kmers_tsv_peak_device_bytes"] <= budget for b in run.batches)


def test_single_pair_defer_patterns(batch_input):
    host = _host(batch_input)
    run = Reduced(batch_input["recs"], batch_input["targets"], defer_patterns=True)
    assert run.hp == b"" and (run.kt, run.kh) == (host.kt, host.kh)
    run.check_stats()


# ---------------------------------------------------------------------------------------------- per-cluster files
@pytest.mark.parametrize("sink,engine_kw", [(None, {}), ("clusters", {}), ("clusters", {"device_gzip_clusters": True})],
                         ids=["no_sink", "cluster_sink", "device_gzip_clusters_cluster_sink"])
def test_multiple_files(batch_input, sink, engine_kw):
    host = _host(batch_input, multiple_files=True, **engine_kw)
    assert len(host.clusters) == 6 and all(kt and kh and hp for _i, kt, kh, hp in host.clusters)
    run = Reduced(batch_input["recs"], batch_input["targets"], sink=sink, multiple_files=True, **engine_kw)
    assert run.clusters == host.clusters
    assert (run.kh, run.hp) == (host.kh, host.hp)
    assert b"".join(c[1] for c in run.clusters) == host.kt
    run.check_stats(multiple_files=True)


# ---------------------------------------------------------------------------------------------- fallback in the middle
@pytest.mark.parametrize("device_gzip", [False, True], ids=["plain", "device_gzip"])
@pytest.mark.parametrize("name_len", [LAST_ON_DEVICE, LAST_ON_DEVICE + 1], ids=["last_on_device", "first_fallback"])
def test_fallback_in_the_middle(batch_input, name_len, device_gzip):
    """three one-cluster batches, the middle one under a cluster name the text kernels lay out (12250 letters at k = 21)
    or refuse (12251): that batch goes through the host renderers, and its rows reach the sink between its neighbours'"""
    from panfeed_amd.engine import GzipMembers
    a, b, c = batch_input["recs"][:3]
    recs = [a, (b[0], "g" * name_len, b[2]), c]
    targets = batch_input["targets"]
    host = Reduced(recs, targets, batch_clusters=1, device_text=False, device_gzip=device_gzip)
    assert all(x["kt"] for x in host.batches)
    run = Reduced(recs, targets, batch_clusters=1, sink="targets", device_gzip=device_gzip)
    assert run.texts() == host.texts()
    assert [x["kt"] for x in run.batches] == [x["kt"] for x in host.batches]      # no batch's rows overtake another's
    fell_back = kh_refused(name_len)
    block = GzipMembers if device_gzip else memoryview
    for i, x in enumerate(run.batches):
        on_host = fell_back and i == 1
        assert x["bodies"] == ((str, str) if on_host else (block, block))
        assert x["sink_kinds"] and set(x["sink_kinds"]) == {str if on_host else block}
        assert x["stats"]["kmers_tsv_streamed"] == len(x["kt"]) == x["sink_text"]
