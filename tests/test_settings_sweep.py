"""Every field of the public settings structs OFF its default: on the device, in the oracle, and in the reference's shader text.

The parity tests elsewhere vary the settings that change the pass list or the inputs; the tuning scalars reach the kernels through the constant buffers and were checked
as bytes only (tests/test_host_constants.py, tests/test_ref_host.py). Here they are checked as arithmetic. tests/settings_cases.py is the table: one entry per field.

  a. completeness   every leaf of the ctypes structs has an entry; a field added to the API later fails until someone decides how it is held
  b. sensitivity    every case moves at least 16 output values of the oracle (a case that moves nothing proves nothing); every `dead` entry moves exactly none
  c. device == oracle, bit for bit, for every one-field case, every twin (siblings with equal defaults at different values) and one all-off-default bundle per family
  d. scalars that change in mid-sequence without changing the pass list (graph mode re-parametrises its cached hipGraphs)
  e. view depth conventions: viewZScale (exact for powers of two), the scale across the denoising range (RELAX votes its tiles on the RAW depth), negated viewZ
  f. oracle == the reference's shader text for the same cases (needs oracle/_ref, as tests/test_ref_parity.py)

CPU: the device sources compiled by tests/emu; GPU: lib/libNRD_hip.so.    python tests/test_settings_sweep.py    prints the sensitivity list
(profiles/settings_sweep_sensitivity.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import parity  # noqa: E402
import settings_cases as sc  # noqa: E402
from oracle import driver as oracle_driver  # noqa: E402
from raytracingdenoiser_amd import api  # noqa: E402

RT = api.ResourceType
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES = 160, 96, 5  # (tests/test_reblur.py / test_relax.py: several workgroups, tiles and LDS windows in both directions)
SENS_W, SENS_H = 96, 64
MIN_MOVED = 16  # not a tolerance: what keeps a case from proving nothing

needs_ref = pytest.mark.skipif(not oracle_driver.ref_available(), reason="oracle/_ref/libnrdref.so not built")


# =========================================================================================================================================== a. completeness
def _ctypes_leaves(struct, prefix):
    out = []
    for field, ctype in struct._fields_:
        path = "%s.%s" % (prefix, field)
        if hasattr(ctype, "_fields_"):
            out += _ctypes_leaves(ctype, path)
        elif hasattr(ctype, "_length_"):
            elem = ctype._type_
            out += sum([_ctypes_leaves(elem, "%s[%d]" % (path, i)) if hasattr(elem, "_fields_") else ["%s[%d]" % (path, i)] for i in range(ctype._length_)], [])
        else:
            out.append(path)
    return out


def test_every_settings_field_has_a_table_entry():
    leaves = [leaf for name, struct in sc.STRUCTS.items() for leaf in _ctypes_leaves(struct, name)]
    assert len(leaves) > 150  # (five 4x4 matrices alone are 80)
    missing = [leaf for leaf in leaves if sc.entry_of(leaf) is None]
    assert not missing, "settings fields that no test decides how to hold: %s" % missing
    stale = [k for k in sc.TABLE if k not in leaves and not any(leaf.startswith(k + "[") for leaf in leaves)]
    assert not stale, "table entries that name no field: %s" % stale
    assert sorted(leaves) == sorted(leaf for name in sc.STRUCTS for leaf in sc.leaves(name))  # (the table's own walk and this one agree)


def test_held_by_entries_name_a_test_file_that_holds_the_field():
    for key, e in sc.TABLE.items():
        if e["kind"] == "held_by":
            path = os.path.join(ROOT, e["path"])
            assert os.path.isfile(path) and os.path.basename(path).startswith("test_"), (key, e["path"])
            field = key.split(".")[1].split("[")[0]
            assert field in open(path).read(), "%s does not mention %s" % (e["path"], field)


def test_the_dead_set_is_exactly_the_fields_no_pass_reads():
    assert sorted(k for k, e in sc.TABLE.items() if e["kind"] == "dead") == ["CommonSettings.debug", "CommonSettings.printfAt",
                                                                             "ReblurSettings.maxStabilizedFrameNumForHitDistance", "RelaxSettings.luminanceEdgeStoppingRelaxation",
                                                                             "SigmaSettings.lightDirection"]


def test_twins_differ_and_bundles_cover_every_case():
    for tag, (family, keys) in sc.TWINS.items():
        values = [sc.TABLE[k]["value"] for k in keys]
        defaults = [getattr(sc.STRUCTS[k.split(".")[0]](), k.split(".")[1]) for k in keys]
        assert len(set(values)) == len(values) and defaults[0] == defaults[1] and not set(values) & set(defaults), tag
    covered = set()
    for name in sc.BUNDLES:
        covered |= set(sc.cases_of(sc.family_of(name)))
    assert covered == {k for k, e in sc.TABLE.items() if e["kind"] == "case"}


# ================================================================================================================================= runs, snapshots, REFERENCE
def _pools(run):
    """every permanent and transient pool plane of a run as raw bytes (the texel bytes of each row, without the pitch padding)"""
    out = {}
    for pool in (RT.PERMANENT_POOL, RT.TRANSIENT_POOL):
        descs = run.inst.permanent_pool if pool == RT.PERMANENT_POOL else run.inst.transient_pool
        for i in range(len(descs)):
            raw, fmt, w = run.ex.pool_plane(pool, i) if hasattr(run.ex, "pool_plane") else run.ex.read_pool_plane(pool, i)
            out[(pool.name, i, fmt.name)] = np.array(raw[:, : w * api.FORMAT_BYTES[fmt]], copy=True)
    return out


def _snapshot(run, pools=True):
    snap = {rt.name: np.array(run.output(rt), copy=True) for rt in run.outs}
    if RT.IN_MV in run.inputs:  # an in/out plane (REBLUR specular motion-vector modification)
        mv = run.inputs[RT.IN_MV]
        snap["IN_MV"] = np.array(mv.cpu().numpy() if hasattr(mv, "cpu") else mv, copy=True)
    if pools:
        snap.update(_pools(run))
    return snap


# The history copies of the view depth hold the host's OWN texels (REBLUR_Blur.hlsli:23 and RELAX_AtrousSmem.hlsli:121-122 store the packed value; the next frame
# unpacks it with viewZScale and abs() again): under a scaled or negated depth plane these planes are the scaled or negated ones, every other plane is the same bytes
DEPTH_COPIES = {"REBLUR_DIFFUSE_SPECULAR": ("PERMANENT_POOL", 0, "R32_SFLOAT"), "RELAX_DIFFUSE_SPECULAR": ("PERMANENT_POOL", 9, "R32_SFLOAT"), "SIGMA_SHADOW": None}


def _assert_same(a, b, what, depth_copy=None, factor=1.0):
    """depth_copy: the key of the pool plane that holds `factor` times the texels of its counterpart in b (exactly: powers of two and signs)"""
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = a[k], b[k]
        if k == depth_copy:
            x, y = np.ascontiguousarray(x).view(np.float32), np.ascontiguousarray(y).view(np.float32) * np.float32(factor)
            assert np.any(x != 0.0), what + (k, "holds no depth")
        same = np.array_equal(x, y, equal_nan=x.dtype.kind == "f")
        assert same, what + (k, "first differing value at", np.argwhere(x != y)[:1].tolist())


def _sequence(name, frames, want=(), edit=None, w=W, h=H):
    seq = parity.generate_sequence(name, w, h, frames, extra_want=want, device="cpu")
    for frame in seq if edit else ():
        edit(frame)
    return seq


def _drive(run, name, seq, args_of, w=W, h=H, pools=True):
    """steps a run through a sequence; args_of(f) = dict(settings_overrides=, cs_kw=) of frame f. Returns one snapshot per frame."""
    snaps = []
    for f, frame in enumerate(seq):
        a = args_of(f)
        cs = parity.common_settings(frame["camera"], seq[max(f - 1, 0)]["camera"], w, h, f, **(a.get("cs_kw") or {}))
        parity.tag_checkerboard(frame, a.get("settings_overrides"), f)
        run.step(frame, cs, parity.denoiser_settings(name, frame, a.get("settings_overrides")))
        snaps.append(_snapshot(run, pools))
    return snaps


def _device(backend):
    if backend == "emu":
        from emu.emu_run import EmuRun

        return EmuRun
    return parity.GpuRun


def _run_alone(make, name, seq, args_of, w=W, h=H):
    """one run from creation to destruction (never two device executors at a time)"""
    run = make(name, w, h)
    try:
        return _drive(run, name, seq, args_of, w, h)
    finally:
        if hasattr(run.ex, "destroy"):
            run.ex.destroy()


REF_W, REF_H = 96, 64


def _reference_signal(f):
    rng = np.random.default_rng(500 + f)
    return (1.0 + rng.random((REF_H, REF_W, 4), dtype=np.float32)).astype(np.float32)


def _reference_run(kind, max_accumulated, frames=FRAMES):
    """the REFERENCE denoiser (a running mean, RGBA32F) with ReferenceSettings::maxAccumulatedFrameNum: the output of every frame and the history plane at the end, as bits"""
    lib = None
    if kind == "emu":
        from emu import emu_run

        lib = emu_run.load()
    inst = api.Instance([(0, api.Denoiser.REFERENCE)], lib=lib)
    if kind == "gpu":
        import torch

        from raytracingdenoiser_amd.executor import HipExecutor

        ex = HipExecutor(inst, REF_W, REF_H)
        out = torch.full((REF_H, REF_W, 4), -7.0, dtype=torch.float32, device="cuda")
        wrap = lambda a: torch.from_numpy(a).cuda()
        host = lambda: out.cpu().numpy()
    else:
        if kind == "emu":
            ex = emu_run.EmuExecutor(inst, REF_W, REF_H)
        else:
            ex = (oracle_driver.RefExecutor if kind == "ref" else oracle_driver.OracleExecutor)(inst, REF_W, REF_H, api.FORMAT_BYTES)
        out = np.full((REF_H, REF_W, 4), -7.0, dtype=np.float32)
        wrap = lambda a: a
        host = lambda: out.copy()
    ex.bind(RT.OUT_SIGNAL, out, api.Format.RGBA32_SFLOAT)
    got, keep = [], []
    for f in range(frames):
        keep.append(wrap(_reference_signal(f)))
        ex.bind(RT.IN_SIGNAL, keep[-1], api.Format.RGBA32_SFLOAT)
        if max_accumulated is not None:
            assert inst.set_denoiser_settings(0, api.ReferenceSettings(maxAccumulatedFrameNum=max_accumulated)) == api.Result.SUCCESS
        cs = api.CommonSettings(resourceSize=(REF_W, REF_H), rectSize=(REF_W, REF_H), resourceSizePrev=(REF_W, REF_H), rectSizePrev=(REF_W, REF_H), timeDeltaBetweenFrames=16.667, frameIndex=f)
        for m in (cs.viewToClipMatrix, cs.viewToClipMatrixPrev, cs.worldToViewMatrix, cs.worldToViewMatrixPrev):
            for k in (0, 5, 10, 15):
                m[k] = 1.0
        assert inst.set_common_settings(cs) == api.Result.SUCCESS
        if kind in ("emu", "gpu"):
            ex.denoise()
        else:
            r, ds = inst.get_compute_dispatches()
            assert r == api.Result.SUCCESS
            ex.execute(ds)
        got.append(host().view(np.uint32))
    raw, fmt, w = ex.read_pool_plane(RT.PERMANENT_POOL, 0) if kind in ("emu", "gpu") else ex.pool_plane(RT.PERMANENT_POOL, 0)
    got.append(np.array(raw[:, : w * api.FORMAT_BYTES[fmt]], copy=True))
    if hasattr(ex, "destroy"):
        ex.destroy()
    return got


def _reference_value():
    return sc.TABLE["ReferenceSettings.maxAccumulatedFrameNum"]["value"]


def _check_reference_bundle(kind):
    want, got = _reference_run("oracle", _reference_value()), _reference_run(kind, _reference_value())
    for f, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), ("REFERENCE", "frame / plane", f)
    # the cap binds: with maxAccumulatedFrameNum = N the weight of frame f is 1 / (1 + min(f, N)), sequential fp32 lerp (REFERENCE_TemporalAccumulation.cs.hlsl:18-27)
    hist = np.zeros((REF_H, REF_W, 4), np.float32)
    for f in range(FRAMES):
        hist = hist + (_reference_signal(f) - hist) * (np.float32(1.0) / (np.float32(1.0) + np.float32(min(f, _reference_value()))))
        assert np.array_equal(want[f], hist.view(np.uint32)), f


# ============================================================================================================================================== b. sensitivity
_oracle_outputs_cache = {}


def _oracle_outputs(name, args, frames):
    """the user outputs (and the in/out plane IN_MV) of every frame of an oracle run at the sensitivity size"""
    key = (name, frames, repr(sorted((k, repr(v)) for k, v in args.items())))
    if key not in _oracle_outputs_cache:
        if name == "REFERENCE":
            _oracle_outputs_cache[key] = _reference_run("oracle", (args.get("settings_overrides") or {}).get("maxAccumulatedFrameNum"), frames)[:-1]
        else:
            seq = _sequence(name, frames, args.get("extra_want", ()), w=SENS_W, h=SENS_H)
            run = parity.OracleRun(name, SENS_W, SENS_H)
            snaps = _drive(run, name, seq, lambda f: args, SENS_W, SENS_H, pools=False)
            _oracle_outputs_cache[key] = [s[k] for s in snaps for k in sorted(s) if k.startswith("OUT_") or k == "IN_MV"]  # (IN_MV is an in/out plane)
    return _oracle_outputs_cache[key]


def _moved(name, on, off, frames):
    a, b = _oracle_outputs(name, on, frames), _oracle_outputs(name, off, frames)
    return sum(int(np.sum(~((x == y) | ((x != x) & (y != y))))) for x, y in zip(a, b)), sum(x.size for x in a)


def sensitivity_rows():
    """(label, moved values, of how many) for every case on every family it runs on, and for both values of every dead entry"""
    rows = []
    for key, e in sc.TABLE.items():
        struct_name = key.split(".")[0]
        if e["kind"] == "case":
            for family in e["on"]:
                moved, n = _moved(sc.BASE[family], sc.build(family, [key]), sc.companions_only(family, [key]), e["frames"])
                rows.append(("case", "%s %s = %r" % (sc.BASE[family], key, e["value"]), moved, n))
        elif e["kind"] == "dead":
            families = sc.ALL3 if struct_name == "CommonSettings" else [f for f, s in sc.STRUCT_OF.items() if s == struct_name]
            for family in families:
                for value in e["values"]:
                    moved, n = _moved(sc.BASE[family], sc.build(family, [key], values={key: value}), sc.companions_only(family, []), FRAMES)
                    rows.append(("dead", "%s %s = %r" % (sc.BASE[family], key, value), moved, n))
    return rows


def test_every_case_moves_the_oracle_and_every_dead_field_moves_nothing():
    rows = sensitivity_rows()
    for kind, label, moved, n in rows:
        print("%-5s %-96s moved %7d of %d" % (kind, label, moved, n))
    weak = [(label, moved) for kind, label, moved, n in rows if kind == "case" and moved < MIN_MOVED]
    alive = [(label, moved) for kind, label, moved, n in rows if kind == "dead" and moved != 0]
    assert not weak, "cases that prove nothing (fewer than %d values moved): %s" % (MIN_MOVED, weak)
    assert not alive, "fields the table calls dead that a pass reads: %s" % alive


# ========================================================================================================================= c. device == oracle, bit for bit
ONE_FIELD = {family: sc.cases_of(family) for family in sc.ALL3}


def _check_parity(name, args, backend, frames=FRAMES):
    worst = parity.run_parity(name, width=W, height=H, frames=frames, check_pools=True, backend=backend, **args)
    assert worst == 0.0, (name, args, worst)


def _check_one_field(family, key, backend):
    _check_parity(sc.BASE[family], sc.build(family, [key]), backend, sc.TABLE[key]["frames"])


def _check_twin(tag, backend):
    family, keys = sc.TWINS[tag]
    _check_parity(sc.BASE[family], sc.build(family, keys), backend)


def _check_bundle(name, backend):
    if name == "REFERENCE":
        return _check_reference_bundle("emu" if backend == "emu" else "gpu")
    _check_parity(name, sc.bundle(name), backend)


@pytest.mark.parametrize("key", ONE_FIELD["REBLUR"])
def test_emulated_reblur_equals_the_oracle_with_one_field_off_its_default(key):
    _check_one_field("REBLUR", key, "emu")


@pytest.mark.parametrize("key", ONE_FIELD["RELAX"])
def test_emulated_relax_equals_the_oracle_with_one_field_off_its_default(key):
    _check_one_field("RELAX", key, "emu")


@pytest.mark.parametrize("key", ONE_FIELD["SIGMA"])
def test_emulated_sigma_equals_the_oracle_with_one_field_off_its_default(key):
    _check_one_field("SIGMA", key, "emu")


@pytest.mark.parametrize("tag", list(sc.TWINS))
def test_emulated_device_equals_the_oracle_with_twin_fields_apart(tag):
    _check_twin(tag, "emu")


@pytest.mark.parametrize("name", sc.BUNDLES)
def test_emulated_device_equals_the_oracle_with_every_field_off_its_default(name):
    _check_bundle(name, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("key", ONE_FIELD["REBLUR"])
def test_reblur_equals_the_oracle_with_one_field_off_its_default(key):
    _check_one_field("REBLUR", key, "hip")


@pytest.mark.gpu
@pytest.mark.parametrize("key", ONE_FIELD["RELAX"])
def test_relax_equals_the_oracle_with_one_field_off_its_default(key):
    _check_one_field("RELAX", key, "hip")


@pytest.mark.gpu
@pytest.mark.parametrize("key", ONE_FIELD["SIGMA"])
def test_sigma_equals_the_oracle_with_one_field_off_its_default(key):
    _check_one_field("SIGMA", key, "hip")


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(sc.TWINS))
def test_device_equals_the_oracle_with_twin_fields_apart(tag):
    _check_twin(tag, "hip")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.BUNDLES)
def test_device_equals_the_oracle_with_every_field_off_its_default(name):
    _check_bundle(name, "hip")


# ================================================================================================================== d. scalars that change in mid-sequence
MID_SEQUENCE = ["REBLUR_DIFFUSE_SPECULAR", "RELAX_DIFFUSE_SPECULAR", "SIGMA_SHADOW"]


def _check_mid_sequence(name, backend, graph=False):
    """frames 0-1 at the defaults, 2-3 with the family's bundle (without the fields whose companions would change the pass list), 4 at the defaults again:
    the pass list is the same for all five, only the constants move"""
    off = sc.bundle(name, mid_sequence=True)
    assert off["settings_overrides"] and off["cs_kw"] and not off["extra_want"]
    args_of = lambda f: off if f in (2, 3) else {}
    seq = _sequence(name, FRAMES)
    dev, ora = _device(backend)(name, W, H), parity.OracleRun(name, W, H)
    if graph:
        dev.ex.set_graph_mode(True)
    lists = []
    for f, frame in enumerate(seq):  # device and oracle in lockstep, compared after every frame
        a = args_of(f)
        for run in (dev, ora):
            cs = parity.common_settings(frame["camera"], seq[max(f - 1, 0)]["camera"], W, H, f, **(a.get("cs_kw") or {}))
            run.step(frame, cs, parity.denoiser_settings(name, frame, a.get("settings_overrides")))
        lists.append([d.shader for d in ora.last_dispatches])
        _assert_same(_snapshot(dev, pools=f == FRAMES - 1), _snapshot(ora, pools=f == FRAMES - 1), (name, "frame", f))
    assert lists[2] == lists[1] and lists[4] == lists[3], "the scalars changed the pass list"


@pytest.mark.parametrize("name", MID_SEQUENCE)
def test_emulated_device_equals_the_oracle_when_only_scalars_change_mid_sequence(name):
    _check_mid_sequence(name, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", MID_SEQUENCE)
def test_device_equals_the_oracle_when_only_scalars_change_mid_sequence(name, graph):
    _check_mid_sequence(name, "hip", graph=graph)


# ========================================================================================================================== e. view depth conventions
DEPTH_NAMES = ["REBLUR_DIFFUSE_SPECULAR", "SIGMA_SHADOW", "RELAX_DIFFUSE_SPECULAR"]
RANGE = 20.0  # a denoising range inside the scene: the far ground and the sky lie beyond it
# the frame size per depth scale: the smallest of the 160-wide sizes at which a whole 16x16 tile lies on different sides of RANGE by raw and by scaled depth (the band of
# ground between RANGE and RANGE / scale is a few rows high: at 160x96 it straddles a tile border for both scales and no tile flips). 104 rows end in half a tile.
RANGE_SIZE = {0.5: (160, 112), 2.0: (160, 104)}
_plain_runs = {}


def _plain(kind, name):
    """the unscaled, positive-depth run of a denoiser on the oracle / a device: computed once, shared by the tests below and left unchanged"""
    if (kind, name) not in _plain_runs:
        make = parity.OracleRun if kind == "oracle" else _device(kind)
        _plain_runs[(kind, name)] = _run_alone(make, name, _sequence(name, FRAMES), lambda f: {})
    return _plain_runs[(kind, name)]


def _scale_depth(factor):
    def edit(frame):
        frame["viewz"] = (frame["viewz"] * factor).contiguous()

    return edit


def _check_scale_invariance(name, kind):
    """viewZ * 2 with viewZScale = 0.5 is the unscaled frame: a power of two scales exactly and the scene has no denormal depths, so every output and every pool plane
    is the same byte for byte (but the history copy of the depth itself: DEPTH_COPIES). Two runs of the same executor kind are compared: device with device, oracle with oracle."""
    make = parity.OracleRun if kind == "oracle" else _device(kind)
    scaled = _run_alone(make, name, _sequence(name, FRAMES, edit=_scale_depth(2.0)), lambda f: dict(cs_kw=dict(viewZScale=0.5)))
    for f, (a, b) in enumerate(zip(scaled, _plain(kind, name))):
        _assert_same(a, b, (name, kind, "frame", f), DEPTH_COPIES[name], 2.0)


def _check_negated_depth(name, backend):
    """a right-handed host hands over negative view depth: every UnpackViewZ takes the magnitude. Device == oracle, and both equal the positive run byte for byte."""
    seq = _sequence(name, FRAMES, edit=_scale_depth(-1.0))
    assert all(float(fr["viewz"].max()) < 0.0 for fr in seq)
    ora = _run_alone(parity.OracleRun, name, seq, lambda f: {})
    dev = _run_alone(_device(backend), name, seq, lambda f: {})
    for f in range(FRAMES):
        _assert_same(dev[f], ora[f], (name, "negated depth, device against oracle, frame", f))
        _assert_same(ora[f], _plain("oracle", name)[f], (name, "negated depth against positive depth, oracle, frame", f), DEPTH_COPIES[name], -1.0)
        _assert_same(dev[f], _plain(backend, name)[f], (name, "negated depth against positive depth, device, frame", f), DEPTH_COPIES[name], -1.0)


def _tiles_all_beyond(depth, limit):
    """per full 16x16 tile: every pixel beyond `limit` (the vote of the ClassifyTiles passes)"""
    h, w = depth.shape
    return (depth[: h // 16 * 16, : w // 16 * 16].reshape(h // 16, 16, w // 16, 16) > limit).all(axis=(1, 3))


def _reaches_the_tile_vote(name, scale, w, h, frames):
    pixels = tiles = 0
    for frame in _sequence(name, frames, w=w, h=h):
        raw = np.abs(frame["viewz"].numpy().reshape(h, w))
        pixels += int(np.sum((raw > RANGE) != (raw * np.float32(scale) > RANGE)))
        tiles += int(np.sum(_tiles_all_beyond(raw, RANGE) != _tiles_all_beyond(raw * np.float32(scale), RANGE)))
    # RELAX_ClassifyTiles.cs.hlsl:37 votes on the RAW |viewZ|, every pass body on the scaled one (REBLUR and SIGMA scale before the vote): the case only reaches
    # that difference if raw and scaled depth fall on different sides of the range somewhere, and if that flips the vote of a whole tile
    assert pixels > 0 and tiles > 0, (name, scale, pixels, tiles)


def _check_scale_across_the_range(name, scale, backend):
    w, h = RANGE_SIZE[scale]
    _reaches_the_tile_vote(name, scale, w, h, FRAMES)
    worst = parity.run_parity(name, width=w, height=h, frames=FRAMES, check_pools=True, backend=backend, cs_kw=dict(denoisingRange=RANGE, viewZScale=scale))
    assert worst == 0.0, (name, scale, worst)


def _check_scale_across_the_range_with_a_shifted_rect(name, scale, backend):
    """the same with CommonSettings::rectOrigin != 0: the device then prepares rect-at-origin guides first and the tile classification runs as a kernel of its own
    (ReblurClassifyTilesKernel / RelaxClassifyTilesKernel) instead of inside the fused decode + classify kernel of the runs above"""
    import ref_parity

    (w, h), origin = RANGE_SIZE[scale], (16, 8)
    resource = (w + 32, h + 16)
    _reaches_the_tile_vote(name, scale, w, h, FRAMES)
    seq = _sequence(name, FRAMES, w=w, h=h)
    dev, ora = _device(backend)(name, *resource), parity.OracleRun(name, *resource)
    for f, fr in enumerate(seq):
        frame = ref_parity.embed_guides_at(fr, resource, origin)
        for run in (dev, ora):
            cs = parity.common_settings(fr["camera"], seq[max(f - 1, 0)]["camera"], w, h, f, resourceSize=resource, resourceSizePrev=resource, rectOrigin=origin,
                                        denoisingRange=RANGE, viewZScale=scale)
            run.step(frame, cs, parity.denoiser_settings(name, frame))
        _assert_same(_snapshot(dev), _snapshot(ora), (name, scale, "shifted rect, frame", f))


@pytest.mark.parametrize("scale", [0.5, 2.0])
@pytest.mark.parametrize("name", ["REBLUR_DIFFUSE_SPECULAR", "RELAX_DIFFUSE_SPECULAR"])
def test_emulated_stand_alone_tile_classification_with_the_depth_scale_across_the_range(name, scale):
    _check_scale_across_the_range_with_a_shifted_rect(name, scale, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [0.5, 2.0])
@pytest.mark.parametrize("name", ["REBLUR_DIFFUSE_SPECULAR", "RELAX_DIFFUSE_SPECULAR"])
def test_stand_alone_tile_classification_with_the_depth_scale_across_the_range(name, scale):
    _check_scale_across_the_range_with_a_shifted_rect(name, scale, "hip")


@pytest.mark.parametrize("name", DEPTH_NAMES)
def test_oracle_is_invariant_under_an_exact_view_depth_scale(name):
    _check_scale_invariance(name, "oracle")


@pytest.mark.parametrize("name", DEPTH_NAMES)
def test_emulated_device_is_invariant_under_an_exact_view_depth_scale(name):
    _check_scale_invariance(name, "emu")


@pytest.mark.parametrize("scale", [0.5, 2.0])
@pytest.mark.parametrize("name", DEPTH_NAMES)
def test_emulated_device_equals_the_oracle_with_the_depth_scale_across_the_range(name, scale):
    _check_scale_across_the_range(name, scale, "emu")


@pytest.mark.parametrize("name", DEPTH_NAMES)
def test_emulated_device_takes_the_magnitude_of_negative_view_depth(name):
    _check_negated_depth(name, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEPTH_NAMES)
def test_device_is_invariant_under_an_exact_view_depth_scale(name):
    _check_scale_invariance(name, "hip")


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [0.5, 2.0])
@pytest.mark.parametrize("name", DEPTH_NAMES)
def test_device_equals_the_oracle_with_the_depth_scale_across_the_range(name, scale):
    _check_scale_across_the_range(name, scale, "hip")


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEPTH_NAMES)
def test_device_takes_the_magnitude_of_negative_view_depth(name):
    _check_negated_depth(name, "hip")


# ============================================================================================================= f. oracle == the reference's shader text
def _ref_cases():
    out = []
    for family in sc.ALL3:
        out += [("%s-%s" % (family, key), sc.BASE[family], sc.build(family, [key])) for key in sc.cases_of(family)]
    out += [("twin-" + tag, sc.BASE[family], sc.build(family, keys)) for tag, (family, keys) in sc.TWINS.items()]
    out += [("bundle-" + name, name, sc.bundle(name)) for name in sc.BUNDLES if name != "REFERENCE"]
    out += [("range-%s-%g" % (name, scale), name, dict(cs_kw=dict(denoisingRange=RANGE, viewZScale=scale), width=RANGE_SIZE[scale][0], height=RANGE_SIZE[scale][1]))
            for name in DEPTH_NAMES for scale in (0.5, 2.0)]
    return out


@needs_ref
@pytest.mark.parametrize("name, args", [pytest.param(name, args, id=tag) for tag, name, args in _ref_cases()])
def test_oracle_matches_the_reference_shader_text_off_the_defaults(monkeypatch, name, args):
    import input_rules
    import ref_parity
    from test_ref_parity import _check  # OK_FLOOR / TOL_FLOOR / EXCEPTIONS of that file, through its own check

    cs_kw = args.get("cs_kw") or {}
    if name in input_rules.OCCLUSION and "denoisingRange" in cs_kw:
        # Without a pre-pass TemporalAccumulation takes the 3x3 minimum of the RAW specular hit distance; the library does not let texels beyond the denoising range into
        # it, the reference does (a documented departure, DESIGN.md 4.2: identical where a host leaves 0 or NaN there). The renderer leaves real hit distances on the
        # ground beyond a range of 20, so this run gets the inputs of a host that clears what it does not want denoised -- tests/input_rules.py, the allowed freedom.
        def clear_beyond_the_range(_, frame, f):
            far = (frame["viewz"].abs() * cs_kw.get("viewZScale", 1.0) > cs_kw["denoisingRange"]).unsqueeze(-1)
            for key in ("diff", "spec"):
                frame[key] = torch.where(far, torch.zeros_like(frame[key]), frame[key]).contiguous()

        import torch

        input_rules.shaped(monkeypatch, clear_beyond_the_range)
    if "width" in args:
        _reaches_the_tile_vote(name, args["cs_kw"]["viewZScale"], args["width"], args["height"], 3)
    _check(ref_parity.run_per_pass(name, frames=3, sensitivity=False, **args), min_rows=10)


@needs_ref
def test_reference_denoiser_matches_the_reference_shader_text_off_the_default():
    for f, (a, b) in enumerate(zip(_reference_run("ref", _reference_value())[:-1], _reference_run("oracle", _reference_value())[:-1])):
        assert np.array_equal(a, b), f


if __name__ == "__main__":
    for kind, label, moved, n in sensitivity_rows():
        print("%-5s %-96s moved %7d of %d" % (kind, label, moved, n))
