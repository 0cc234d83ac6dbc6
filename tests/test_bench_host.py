"""bench.py's host-side arithmetic, no GPU: where `roofline.traffic` and `roofline.pipes.valu_insts_per_block` come from
(VERDICT r04 #8a / ADVICE r04: the VALU-per-block figure was a constant copied by hand and went stale with the next
kernel change -- it is now derived from the SQ_INSTS_VALU pass of the same run, or quoted from profiles/pmc_valu.json
with its provenance when no pass can run)."""
import json
import os

import bench

GIB = 1 << 30


def test_valu_per_block_is_derived_from_the_runs_own_counter_pass():
    # 2.237e8 wave instructions per 1 GiB step (profiles/r04_ctr_rocprof_summary.txt) -> 213 per block
    v, src = bench.valu_per_block_of({"SQ_INSTS_VALU": 2.237e8}, GIB, "ctr")
    assert abs(v - 213.3) < 0.2 and src.startswith("measured in this run")
    v2, _ = bench.valu_per_block_of({"SQ_INSTS_VALU": 2.0e8}, GIB, "ctr")       # a different kernel -> a different figure
    assert abs(v2 - 190.7) < 0.2


def test_valu_per_block_falls_back_to_the_recorded_figure_and_says_so(tmp_path):
    with open(os.path.join(bench.ROOT, "profiles", "pmc_valu.json")) as f:
        rec = json.load(f)
    for wl in ("ctr", "gcm", "xts"):
        v, src = bench.valu_per_block_of({}, GIB, wl)
        assert v == rec[wl]["valu_insts_per_block"] and src.startswith("recorded in profiles/") and "not measured in this run" in src
        assert os.path.exists(os.path.join(bench.ROOT, rec[wl]["source"]))
    assert bench.valu_per_block_of({}, GIB // 2, "ctr") == (None, None)            # another size: no figure rather than a stale one
    assert bench.valu_per_block_of({}, GIB, "ecb") == (None, None)
    (tmp_path / "pmc_valu.json").write_text(json.dumps({"ctr": {"bytes_per_gpu": GIB, "valu_insts_per_block": 7,
                                                                "source": "x", "build": "y"}}))
    assert bench.valu_per_block_of({}, GIB, "ctr", str(tmp_path))[0] == 7


def test_traffic_from_the_two_counter_passes():
    t, src = bench.traffic_of({"FETCH_SIZE": 527966.0, "WRITE_SIZE": 1059605.0})
    assert t == int((2 * 527966 + 1059605) * 1024) and src.startswith("measured in this run")
    assert bench.traffic_of({"FETCH_SIZE": 1.0}) == (None, None)


def test_a_plain_run_does_only_what_value_needs_and_full_adds_the_rest():
    ap = bench.build_parser()
    plain = bench.resolve_extras(ap.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "3"]))
    assert not plain.full and plain.sustain_s == 0.0
    assert plain.no_verify and plain.no_traffic and plain.no_other_configs and plain.no_cpu
    assert bench.resolve_gather_flags(plain, 1) == (False, False) and bench.resolve_gather_flags(plain, 8) == (False, False)
    full = bench.resolve_extras(ap.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "3", "--full"]))
    assert full.sustain_s == 2.0
    assert not (full.no_verify or full.no_traffic or full.no_other_configs or full.no_cpu)
    assert bench.resolve_gather_flags(full, 8) == (True, True) and bench.resolve_gather_flags(full, 1, force=True) == (True, True)
    # under --full a --no-* switch still turns its part off; an explicit --sustain-s holds with or without --full
    some = bench.resolve_extras(ap.parse_args(["--full", "--no-cpu", "--sustain-s", "0"]))
    assert some.no_cpu and not some.no_verify and some.sustain_s == 0.0
    assert bench.resolve_extras(ap.parse_args(["--sustain-s", "0.5"])).sustain_s == 0.5
