"""The oracle against the reference's own shader text (tests/test_ref_parity.py: every pass on identical inputs, the same statistics and the same floors) on the inputs of
tests/test_input_rules.py that NRD's input rules allow and the synthetic renderer never produces: NaN in the noisy inputs beyond the denoising range, arbitrary finite guides on
the sky, a sky made by viewZ alone over texels that keep a geometry normal and a signal. The GPU tests hold the library to the oracle on these inputs bit for bit; this hop says
that the oracle's answer on them is the reference's.

It also settles what the dirty guides do: with finite garbage in the sky texels' normals and roughness the outputs on GEOMETRY change -- and the oracle still equals the
reference text pass by pass. The reference's spatial filters weigh a tap by the tap texel's normal, roughness and viewZ-derived plane distance without asking whether that texel
is inside the range, so a host's sky guides take part in the result next to the horizon: that is the reference's behaviour, and no invariance is claimed for guides."""
import pytest

import input_rules
import ref_parity
from test_ref_parity import _check, pytestmark  # noqa: F401  (skipped where oracle/_ref is not built)

MAIN = ["REBLUR_DIFFUSE_SPECULAR", "RELAX_DIFFUSE_SPECULAR_SH", "SIGMA_SHADOW"]
SHAPES = {
    "nan_sky": lambda name, frame, f: input_rules.dirty_sky_noisy(frame, "nan", f, name),
    "dirty_guides": lambda name, frame, f: input_rules.dirty_sky_guides(frame),
    "painted_sky": lambda name, frame, f: input_rules.paint_sky(frame, f, True),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", MAIN)
def test_every_pass_matches_the_reference_shader_text_on_inputs_the_rules_allow(monkeypatch, name, shape):
    input_rules.shaped(monkeypatch, SHAPES[shape])
    rows = _check(ref_parity.run_per_pass(name, frames=3, sensitivity=False), min_rows=10)
    if name.startswith("SIGMA"):
        assert all(r["bit_exact_frac"] == 1.0 for r in rows)
