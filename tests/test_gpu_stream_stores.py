"""The root pass inside the boundary launch stores its root terms write-through, a few per K-step under two staggered MFMA chains
(csrc/bg_root_resident.h, bg_stream_store.h).  Results must stay what they were, bit for bit: the paced in-launch pass against the
stand-alone root pass (plain stores, a tile at a time) at the smallest fused size, with ragged last workgroups.  Small envs, the
stand-alone pass and the expansion's rows are not touched by that change: tests/test_gpu_parity.py covers them as before."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FUSED_FROM = 24576                     # lanes from which run_greedy moves the root pass into the boundary launch


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


# 37 games in the env's last workgroup of 128: two tiles, the second partial; 70 games: three tiles, the odd case
@pytest.mark.parametrize("extra", [37, 70])
def test_paced_root_pass_in_boundary_equals_stand_alone_pass(bg, weights, extra):
    """run_greedy(k) (steps 2 .. k take their root terms from the boundary launch of the step before) against k calls of step_greedy (every
    step: roots_kernel + root_hidden_resident_kernel + apply_kernel), after every step k = 1 .. 6: snapshot and last choice bit for bit."""
    n, seed, steps = FUSED_FROM + extra, 4711, 6
    b = bg.VecGame(n, seed=seed)
    b.load_weights(weights)
    a = None
    for k in range(1, steps + 1):
        a = bg.VecGame(n, seed=seed)                  # a fresh env per k: its k steps are ONE run
        a.load_weights(weights)
        a.run_greedy(k)
        b.step_greedy()
        assert torch.equal(a.snapshot(), b.snapshot()), k
        la, lb = a.last_choice(), b.last_choice()
        for key in ("chosen", "count", "seq", "seq_len"):
            assert torch.equal(la[key], lb[key]), (k, key)
        assert torch.equal(la["value"].view(torch.int32), lb["value"].view(torch.int32)), k
    sa, sb = a.stats(), b.stats()
    assert sa == sb, (sa, sb)
    assert sa["error_flags"] == 0
