"""The learner's three routes on the device, entry by entry (backgammon_env/learner.py: replay_route, _issue): the update applied by the
library (LOCAL), by the Python-driven step / apply loop (split_apply: TORCH on one rank, no collective) and through the learner's own
RCCL communicator on a world of one (LIBRARY) leave the same weights and the same statistics, bit for bit; a game table with one game
per lane IS the streamed replay of the rows.  One 64-lane round, no process group.  (tests/test_replay_route_cpu.py has what cannot be
run here: more ranks, the torch collectives, every combination of the settings.)"""
import gc

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 64
ENTRIES = {
    "rows": (("local", "split_apply", "library"), {}),
    "rows sub_round=16": (("local", "split_apply", "library"), {"sub_round": 16}),
    "rows slots=7": (("local", "split_apply", "library"), {"slots": 7}),
    "games slots=7": (("local", "library"), {"slots": 7}),
    "fit_step": (("local", "library"), {}),
}


@pytest.fixture(scope="module")
def runs(weights):
    """{(entry, route): ((Σ δ², count[, skipped]), theta)} of the thirteen cases, each on a learner of its own"""
    import backgammon_env as bg
    from backgammon_env.learner import DeviceTDLambdaLearner, play_round
    env = bg.VecGame(N, seed=21)
    env.load_weights(weights)
    rows, lengths, won = play_round(env, max_plies=400, epsilon=0.05)
    assert int((lengths > 0).sum().item()) > 7                    # more games than slots: the slots do take game after game
    lane = torch.arange(N, dtype=torch.int32, device=rows.device)
    out = {}
    mp = pytest.MonkeyPatch()
    try:
        for entry, (routes, kw) in ENTRIES.items():
            for route in routes:
                mp.delenv("BGAMD_FORCE_COLLECTIVE", raising=False)
                mp.delenv("BGAMD_TD_TORCH_COLLECTIVE", raising=False)
                L = DeviceTDLambdaLearner(weights, max_games=N, alpha=0.1, lam=0.7)
                if route == "library":
                    L.init_collective()
                    assert L._comm == (0, 1)
                    mp.setenv("BGAMD_FORCE_COLLECTIVE", "1")
                assert L._route(None, route == "split_apply").kind == {"local": "local", "split_apply": "torch", "library": "library"}[route]
                if entry == "fit_step":
                    L.fit_step(rows[0], won.to(torch.float32))
                    stats = L.fit_stats()
                elif entry.startswith("games"):
                    stats = L.replay_games(rows, lane, torch.zeros_like(lane), lengths, won, **kw)
                else:
                    stats = L.replay_rows(rows, lengths, won, split_apply=route == "split_apply", **kw)
                out[entry, route] = (stats, L.theta.clone())
                del L
                gc.collect()
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_an_entrys_routes_agree_bit_for_bit(runs, entry):
    routes = ENTRIES[entry][0]
    stats, theta = runs[entry, routes[0]]
    assert stats[1] > 0
    for route in routes[1:]:
        assert runs[entry, route][0] == stats, (entry, route)
        assert torch.equal(runs[entry, route][1], theta), (entry, route)


def test_a_table_of_one_game_per_lane_is_the_streamed_replay_of_the_rows(runs):
    for route in ENTRIES["games slots=7"][0]:
        assert runs["games slots=7", route][0] == runs["rows slots=7", route][0]
        assert torch.equal(runs["games slots=7", route][1], runs["rows slots=7", route][1])


def test_every_case_moved_the_weights(runs, weights):
    assert len(runs) == 13
    w = torch.as_tensor(weights, device="cuda")
    for key, (_, theta) in runs.items():
        assert (theta - w).abs().max().item() > 1e-4, key
