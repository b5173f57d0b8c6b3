"""WeightCache (svdd_amd/diffusion.py): the one rule that keeps re-packed copies of weights from going stale, with plain
nn.Modules and a counting build — no GPU, no fused net."""
import gc

import torch
from torch import nn

from svdd_amd import diffusion
from svdd_amd.diffusion import WeightCache


class _Counting:
    """A build callback that counts its calls and returns a fresh object each time."""

    def __init__(self, result=object):
        self.calls, self.result = 0, result

    def __call__(self):
        self.calls += 1
        return self.result()


def _count_fingerprints(monkeypatch):
    calls = []
    real = diffusion.weight_fingerprint

    def counted(*modules, **kw):
        calls.append(modules)
        return real(*modules, **kw)
    monkeypatch.setattr(diffusion, "weight_fingerprint", counted)
    return calls


def test_one_validation_per_scope(monkeypatch):
    fps = _count_fingerprints(monkeypatch)
    cache, lin, build = WeightCache(), nn.Linear(4, 4), _Counting()
    a = cache.get("k", (lin,), build, scope=1)
    assert (build.calls, len(fps), len(cache)) == (1, 1, 1)
    for _ in range(3):                                              # the per-step path: same scope, no fingerprint
        assert cache.get("k", (lin,), build, scope=1) is a
    assert (build.calls, len(fps)) == (1, 1)
    assert cache.get("k", (lin,), build, scope=2) is a              # next decode: one fingerprint, same weights, no rebuild
    assert (build.calls, len(fps)) == (1, 2)
    assert cache.get("k", (lin,), build, scope=2) is a
    assert (build.calls, len(fps)) == (1, 2)
    assert cache.get("other", (lin,), build, scope=2) is not a      # the kind is part of the key
    assert (build.calls, len(cache)) == (2, 2)


def test_every_kind_of_weight_change_rebuilds_once_at_the_next_scope():
    cache, lin, build = WeightCache(), nn.Linear(4, 4), _Counting()
    scope = 1
    last = cache.get("k", (lin,), build, scope)

    def changed():
        """The change is not seen inside the running scope; the next scope rebuilds exactly once."""
        nonlocal scope, last
        n = build.calls
        assert cache.get("k", (lin,), build, scope) is last and build.calls == n
        scope += 1
        new = cache.get("k", (lin,), build, scope)
        assert new is not last and build.calls == n + 1
        assert cache.get("k", (lin,), build, scope) is new and build.calls == n + 1
        scope += 1
        assert cache.get("k", (lin,), build, scope) is new and build.calls == n + 1       # unchanged since: no rebuild
        last = new

    with torch.no_grad():
        lin.bias.add_(0.25)
    changed()
    lin.load_state_dict({k: v.clone() + 1.0 for k, v in lin.state_dict().items()})
    changed()
    v = lin.weight._version
    lin.weight.data.copy_(lin.weight.data * 0.5)                    # the EMA swap: no version bump, only the content moves
    assert lin.weight._version == v
    changed()

    # outside any scope every call validates: a change is seen at the very next call
    n = build.calls
    a = cache.get("k", (lin,), build, None)
    assert a is last and build.calls == n
    lin.weight.data.copy_(lin.weight.data * 0.5)
    b = cache.get("k", (lin,), build, None)
    assert b is not a and build.calls == n + 1
    assert cache.get("k", (lin,), build, None) is b and build.calls == n + 1


def test_outside_a_scope_every_call_fingerprints(monkeypatch):
    fps = _count_fingerprints(monkeypatch)
    cache, lin, build = WeightCache(), nn.Linear(4, 4), _Counting()
    for _ in range(3):
        cache.get("k", (lin,), build, None)
    assert (build.calls, len(fps)) == (1, 3)
    cache.get("k", (lin,), build, 7)                                # an entry stamped outside a scope is not trusted inside one
    assert (build.calls, len(fps)) == (1, 4)


def test_a_collected_module_never_hands_its_value_to_a_new_one():
    cache, keep = WeightCache(), nn.Linear(4, 4)
    kept = cache.get("k", (keep, keep), object, scope=1)
    for _ in range(50):                                             # CPython hands a freed module's id() to the next one
        torch.manual_seed(0)                                        # same weights every time: only identity tells them apart
        lin = nn.Linear(4, 4)
        token = object()
        assert cache.get("k", (lin, keep), lambda: token, scope=1) is token       # never a dead module's value
        assert len(cache) == 2                                      # the dead entry went when the new one was built
        del lin
        gc.collect()
    assert cache.get("k", (keep, keep), object, scope=1) is kept    # entries of living modules are not purged


def test_a_build_that_returns_none_is_cached():
    cache, lin = WeightCache(), nn.Linear(4, 4)
    build = _Counting(result=lambda: None)
    assert cache.get("k", (lin,), build, scope=1) is None
    assert cache.get("k", (lin,), build, scope=1) is None
    assert cache.get("k", (lin,), build, scope=2) is None
    assert (build.calls, len(cache)) == (1, 1)


def test_clear_and_clear_fused_leave_nothing_behind():
    cache, lin = WeightCache(), nn.Linear(4, 4)
    cache.get("a", (lin,), object, 1), cache.get("b", (lin,), object, 1)
    assert len(cache) == 2
    cache.clear()
    assert len(cache) == 0

    from svdd_amd.config import dna_config
    d = diffusion.Diffusion(dna_config(hidden_dim=16, num_cnn_stacks=1)).eval()
    assert isinstance(d._fused, WeightCache) and len(d._fused) == 0
    declared = set(vars(d))
    gru = nn.GRU(64, 64, batch_first=True, bidirectional=True)
    for kind, modules in (("backbone", (d.backbone,)), ("value", (lin, gru)), (("trunk", "bf16"), (lin, gru)), ("gru_packs", (gru,))):
        d._fused.get(kind, modules, object, d._scope)
    d._validate_conv_packs()                                        # the fifth kind, through its own call site
    d.backbone._cpk_key = "packed"
    assert len(d._fused) == 5
    d.clear_fused()
    assert len(d._fused) == 0 and d.backbone._cpk_key is None
    assert set(vars(d)) == declared                                 # no cache in an attribute __init__ does not declare
    build = _Counting()
    d._fused.get("gru_packs", (gru,), build, d._scope)              # ... so everything is rebuilt
    assert build.calls == 1
