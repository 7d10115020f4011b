"""The legacy Transception network (networks/Transception.py) on the host side, no GPU: constructor, state_dict schema against the
reference's (tests/golden/legacy.npz), seeded initialisation, strict loads both ways, refused configurations."""
import inspect

import numpy as np
import pytest
import torch

from golden_util import load
from transception_amd.seeded_init import schema_digest, schema_entries, seeded_state_dict

CONFIGS = {"default": {}, "sk": dict(concat="sk"), "nodil": dict(dil_conv=0), "heads8": dict(head_count=8), "mix": dict(token_mlp_mode="mix")}


@pytest.fixture(scope="module")
def gold():
    return load("legacy.npz")


def _text(a) -> str:
    return bytes(a.tobytes()).decode()


def test_exported_next_to_the_alias():
    import transception_amd
    from transception_amd import MSTransception, Transception, TransCeption
    assert "Transception" in transception_amd.__all__
    assert TransCeption is MSTransception and Transception is not MSTransception


def test_constructor_defaults_are_the_reference_ones():
    from transception_amd import Transception
    sig = inspect.signature(Transception.__init__).parameters
    assert {k: v.default for k, v in sig.items() if k != "self"} == dict(num_classes=9, head_count=1, dil_conv=1, token_mlp_mode="mix_skip",
                                                                         concat="original")


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_schema_matches_reference(gold, cfg):
    from transception_amd import Transception
    m = Transception(num_classes=9, **CONFIGS[cfg])
    entries = schema_entries(m)
    assert [k for k, _, _ in entries] == _text(gold[cfg + "/keys"]).split("\n")
    assert schema_digest(entries) == _text(gold[cfg + "/schema_sha256"])
    assert [len(entries), len({c for _, _, c in entries})] == gold[cfg + "/n_keys"].tolist()
    if cfg != "mix":
        assert len(entries) == 561 and len(list(m.parameters())) == 552
        assert sum(p.numel() for p in m.parameters()) == 30004009


def test_seeded_init_is_the_reference_init(gold):
    from transception_amd import Transception
    torch.manual_seed(1234)
    sd = Transception().state_dict()
    assert list(sd) == _text(gold["init/keys"]).split("\n")
    sums = np.array([float(t.double().sum()) for t in sd.values()])
    np.testing.assert_array_equal(sums, gold["init/sums"])


def test_strict_load_both_ways():
    from transception_amd import Transception
    a = Transception(concat="sk")
    sd = seeded_state_dict(schema_entries(a))
    a.load_state_dict(sd, strict=True)
    b = Transception(concat="sk")
    b.load_state_dict(a.state_dict(), strict=True)
    for k, v in b.state_dict().items():
        assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("kw", [dict(head_count=3), dict(token_mlp_mode="mlp")])
def test_unsupported_configurations_raise(kw):
    from transception_amd import Transception
    with pytest.raises(NotImplementedError):
        Transception(**kw)


def test_cpu_input_has_no_fallback():
    from transception_amd import Transception
    m = Transception()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 224, 224))


def test_other_sizes_are_refused():
    from transception_amd import Transception
    with pytest.raises(ValueError):
        Transception()(torch.zeros(1, 1, 256, 256))


def test_no_split_backward():
    from transception_amd import Transception
    with pytest.raises(NotImplementedError):
        Transception().gradient_pieces()
