"""CPU checks of small pieces the measurements and the multi-GPU defaults rest on (no GPU, no oracle)."""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_history_halo_default_scales_with_the_frame_height():
    from raytracingdenoiser_amd import sharding

    rows = [sharding.HaloSharder.default_motion_rows(h) for h in (128, 720, 1080, 1440, 2160, 4320)]
    assert rows == [32, 32, 32, 32, 48, 96]  # 32 up to 1440p (the value every committed measurement used), proportional above
    assert rows == sorted(rows)


def test_counter_summaries_fold_into_valu_figures():
    """tools/pmc_to_json.py on the committed counter summaries: the per-kernel VALU figures bench.py's roofline.valu is built from"""
    import pmc_to_json

    sq = pmc_to_json.parse_columns(os.path.join(ROOT, "profiles", "r03_i_reblur_ds_pmc3.txt"))
    ta = [v for k, v in sq.items() if "ReblurTemporalAccumulationKernel<true, true, false, 0, false, 3, 1>" in k]
    assert len(ta) == 1 and ta[0]["SQ_WAVES"] == 57600.0  # 2560 x 1440 / 64
    per_wave = ta[0]["SQ_INSTS_VALU"] / ta[0]["SQ_WAVES"]
    assert 2000 < per_wave < 3000
    cycles_per_instruction = 4.0 * ta[0]["SQ_ACTIVE_INST_V"] / ta[0]["SQ_INSTS_VALU"]  # the counter's unit is 4 cycles
    assert 3.9 < cycles_per_instruction < 4.4
    fetch = pmc_to_json.parse(os.path.join(ROOT, "profiles", "r03_i_reblur_ds_pmc1.txt"))
    assert any("ReblurSpatialKernel" in k for k in fetch) and all(v >= 0 for v in fetch.values())


def test_lds_array_pricing_prefers_whole_texel_reads():
    """tools/isa_stats.py: the rule that found RELAX HistoryClamping's bound -- a float4 texel read as b96 + b32 costs 4x one b128"""
    import isa_stats

    split = collections.Counter({"ds_read_b96": 102, "ds_read_b32": 51})
    whole = collections.Counter({"ds_read_b128": 104})
    assert isa_stats.lds_cycles(whole) == 416
    assert isa_stats.lds_cycles(split) >= 2 * isa_stats.lds_cycles(whole)  # (conflict-free pricing; the b32 reads at a 16-byte stride conflict 4-way on top)


def test_listing_comparison_tells_moved_labels_from_changed_instructions(tmp_path, capsys):
    """tools/isa_stats.py --identical, the check a refactoring of the device sources is held to: a kernel whose block labels only carry another function index is
    the same kernel; another instruction, or another register count, is not; kernels present on one side only are counted, not compared."""
    import isa_stats

    def listing(index, add, vgprs, extra=""):
        kernel = "\n_Z1kv:\n\ts_load_dword s0, s[0:1], 0x0\n.LBB%d_1:\n\t%s v0, v0, v1\n\ts_cbranch_scc1 .LBB%d_1\n\ts_endpgm\n.Lfunc_end%d:\n; NumVgprs: %d\n; Occupancy: 8\n; ScratchSize: 0\n; LDSByteSize: 0\n"
        return "\t.text\n" + extra + kernel % (index, add, index, index, vgprs)

    gone = "\n_Z4gonev:\n\ts_endpgm\n.Lfunc_end0:\n; NumVgprs: 1\n; Occupancy: 8\n; ScratchSize: 0\n; LDSByteSize: 0\n"
    for name, text in (("old", listing(1, "v_add_f32_e32", 2, gone)), ("moved", listing(0, "v_add_f32_e32", 2)), ("changed", listing(0, "v_mul_f32_e32", 2)), ("fatter", listing(0, "v_add_f32_e32", 3))):
        (tmp_path / (name + ".s")).write_text(text)
    assert isa_stats.identical([str(tmp_path / "old.s"), str(tmp_path / "moved.s")]) == 0
    assert "identical 1, removed 1, added 0, differing 0" in capsys.readouterr().out
    assert isa_stats.identical([str(tmp_path / "old.s"), str(tmp_path / "changed.s")]) == 1
    assert isa_stats.identical([str(tmp_path / "old.s"), str(tmp_path / "fatter.s")]) == 1


def test_every_environment_switch_of_the_library_is_documented():
    """The names the native sources hand to getenv are exactly the NRD_HIP_* switches INTEGRATION.md lists in its paragraph on the library's environment switches:
    a switch nobody can look up is either undocumented or dead."""
    import re

    read = set()
    for d, _, files in os.walk(os.path.join(ROOT, "raytracingdenoiser_amd", "csrc")):
        for f in files:
            read |= set(re.findall(r'getenv\(\s*"([^"]+)"', open(os.path.join(d, f)).read()))
    bullets = [b for b in re.split(r"\n(?=\* )", open(os.path.join(ROOT, "INTEGRATION.md")).read()) if "(environment, read once per process" in b]
    assert len(bullets) == 1
    documented = set(re.findall(r"NRD_HIP_[A-Z0-9_]+", bullets[0].split("\n\n")[0]))
    assert read == documented, (sorted(read - documented), sorted(documented - read))
