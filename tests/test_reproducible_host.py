"""Host side of the reproducible mode (ops.set_reproducible): ABI numbers, the workspace query, the per-thread switch."""
import os
import re
import subprocess
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_agree_on_abi_29():
    from position_induced_transformer_amd import _lib
    with open(os.path.join(ROOT, "include", "pit_hip.h")) as f:
        m = re.search(r"#define\s+PIT_ABI_VERSION\s+(\d+)", f.read())
    assert m and int(m.group(1)) == _lib.ABI_VERSION >= 29
    for name in ("pit_mlp_bwd_params_ordered_mfma", "pit_mlp_bwd_params_ordered_mfma_workspace", "pit_lists_sort_ranges",
                 "pit_posatt_overflow_dv_ordered"):
        assert name in _lib.SIGNATURES
    assert "pit_mlp_bwd_params_ordered_mfma_workspace" in _lib.LONG_RETURN


def test_workspace_query():
    from position_induced_transformer_amd import _lib
    q = _lib.lib().pit_mlp_bwd_params_ordered_mfma_workspace
    for rows, n0, n1, n2 in [(1, 3, 32, 32), (4099, 192, 64, 64), (300, 768, 256, 256), (9720, 44, 128, 1)]:
        per_slab = (n1 * n0 + n1 + n2 * n1 + n2) * 4
        got = q(rows, n0, n1, n2)
        assert got > 0 and got % per_slab == 0 and 1 <= got // per_slab <= 64, (rows, n0, n1, n2, got)
        assert got == q(rows, n0, n1, n2)                # a pure function of the sizes
    assert q(1, 3, 32, 32) == (32 * 3 + 32 + 32 * 32 + 32) * 4          # one row: one slab
    for bad in [(0, 3, 32, 32), (-5, 3, 32, 32), (10, 0, 32, 32), (10, 3, 0, 32), (10, 3, 32, 0), (10, 3, 32, -1)]:
        assert q(*bad) == 0, bad


def test_switch_is_per_thread():
    from position_induced_transformer_amd import ops
    seen = {}
    gate_on, gate_done = threading.Event(), threading.Event()

    def on_thread():
        ops.set_reproducible(True)
        seen["on"] = ops.get_reproducible()
        gate_on.set()
        gate_done.wait(10)

    def other_thread():
        gate_on.wait(10)
        seen["other"] = ops.get_reproducible()
        gate_done.set()

    before = ops.get_reproducible()
    ts = [threading.Thread(target=on_thread), threading.Thread(target=other_thread)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(20)
    assert seen == {"on": True, "other": before}
    assert ops.get_reproducible() == before


@pytest.mark.parametrize("value,expect", [("1", True), ("0", False), (None, False)])
def test_switch_follows_the_environment_in_a_fresh_process(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "PIT_REPRODUCIBLE"}
    if value is not None:
        env["PIT_REPRODUCIBLE"] = value
    code = "from position_induced_transformer_amd import ops; print(ops.get_reproducible())"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip().splitlines()[-1] == str(expect)


def test_context_manager_restores_after_an_exception():
    from position_induced_transformer_amd import ops
    before = ops.get_reproducible()
    with pytest.raises(KeyError):
        with ops.reproducible():
            assert ops.get_reproducible() is True
            with ops.reproducible(False):
                assert ops.get_reproducible() is False
            assert ops.get_reproducible() is True
            raise KeyError("x")
    assert ops.get_reproducible() == before


def test_bf16_math_mode_is_refused():
    from position_induced_transformer_amd import ops
    with ops.math_mode("bf16"), ops.reproducible():
        with pytest.raises(NotImplementedError, match="reproducible"):
            ops.reproducible_wanted()
    with ops.math_mode("bf16"):
        assert ops.reproducible_wanted() is False
