"""The drop-in claim, checked against the reference's own model files through what they produce: after `dropin.install()` every
`mamba_ssm` / `causal_conv1d` name the reference's `mamba_simple.py` files import resolves to this package, and the modules the
reference builds have the same parameter names and shapes as the mirror's, i.e. checkpoints move both ways.  The reference's layouts
(state_dict names and shapes of each module below) are recorded in tests/golden/dropin_reference.json by
`python tests/golden/make_golden.py dropin_reference`, which loads the reference's files on top of the drop-in.  Construction only: CPU."""
import importlib
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dropin_reference.json")

# the third-party names the reference's mamba_simple.py files import (dropin.py's docstring), by module
DROPIN_NAMES = {
    "causal_conv1d": ("causal_conv1d_fn", "causal_conv1d_update"),
    "mamba_ssm.ops.selective_scan_interface": ("selective_scan_fn", "mamba_inner_fn", "mamba_inner_fn_no_out_proj"),
    "mamba_ssm.ops.triton.selective_state_update": ("selective_state_update",),
}


@pytest.fixture(autouse=True)
def _restore_sys_modules():
    """The drop-in registers modules under third-party names; later tests (transformers probes `find_spec("timm")`) must not see them."""
    before = dict(sys.modules)
    yield
    for k in list(sys.modules):
        if k not in before:
            del sys.modules[k]
    sys.modules.update({k: v for k, v in before.items() if sys.modules.get(k) is not v})


def _recorded(case):
    with open(GOLDEN) as f:
        rec = json.load(f)
    return {k: tuple(v) for k, v in rec["layouts"][case].items()}, rec


def _layout(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def _check_dropin_names():
    import medical_image_analysis_amd.dropin as dropin
    dropin.install()
    for mod, names in DROPIN_NAMES.items():
        m = importlib.import_module(mod)
        for name in names:
            assert getattr(m, name).__module__.startswith("medical_image_analysis_amd."), (mod, name)


def _reference_checkpoint(layout):
    """A state_dict in the reference's layout (the values do not matter to a strict load)."""
    g = torch.Generator().manual_seed(0)
    return {k: torch.randn(shape, generator=g) for k, shape in layout.items()}


@pytest.mark.parametrize("bimamba_type", ["v2", "v3", "v4"])
def test_reference_finetuning_mamba_imports_and_matches_layout(bimamba_type):
    from medical_image_analysis_amd.mamba_simple import Mamba
    _check_dropin_names()
    theirs, _ = _recorded(f"finetuning_mamba_{bimamba_type}")
    mine = Mamba(d_model=48, bimamba_type=bimamba_type)
    assert _layout(mine) == theirs
    mine.load_state_dict(_reference_checkpoint(theirs), strict=True)        # a reference checkpoint loads


def test_reference_pretrain_mamba_imports_and_matches_layout():
    from medical_image_analysis_amd.mamba_simple import Mamba
    _check_dropin_names()
    theirs, _ = _recorded("pretrain_mamba")
    mine = Mamba(d_model=64, expand=1, bimamba_type="None")
    assert _layout(mine) == theirs


def test_reference_arm_encoder_layout_equals_mirror():
    """The reference's `arm_base_pz16` (arm/Finetuning/models_mamba.py:398-410) built on top of the drop-in ops next to the
    mirror's: identical state_dict keys and shapes, strict load of a checkpoint in the reference's layout."""
    from medical_image_analysis_amd import models_mamba as mine_mod
    theirs, rec = _recorded("arm_encoder")
    mine = mine_mod.arm_base_pz16("base")
    assert _layout(mine) == theirs
    mine.load_state_dict(_reference_checkpoint(theirs), strict=True)
    ref = rec["arm_encoder"]
    assert mine.num_features == ref["num_features"] == 768 and mine.patch_embed.num_patches == ref["num_patches"] == 196


def test_reference_pretrain_model_layout_equals_mirror():
    """`pretrain/models_pretrain.py` arm_base_pz16 (stage-1 VisionMamba, :518-527) likewise."""
    from medical_image_analysis_amd import models_pretrain as mine_mod
    theirs, _ = _recorded("pretrain_model")
    mine = mine_mod.arm_base_pz16()
    assert _layout(mine) == theirs
    mine.load_state_dict(_reference_checkpoint(theirs), strict=True)
