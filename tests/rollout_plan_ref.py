"""An independent restatement of what a call of bgamd_env_rollout_grouped decides before and while it issues anything, for
tests/test_rollout_plan_cpu.py to hold csrc/bg_rollout_plan.h against.  Written from the rollout section of include/bgamd.h and from the
text of the entry point as it stood in the commit before the header existed (its argument checks in their order, its locals F, n_fan, L,
R, G, the sizes it passed to its scratch envs and to its ten grow calls, its loop's stall count), not from the header.  No device, no
numpy: plain integers.

A request is the tuple (flags, P, offset, T, M, lanes, has_states, has_group, plies, top_k, cube, w0, w1), as the driver reads it."""
ROTATE, SLOT1, VR = 128, 64, 256                        # include/bgamd.h
OK, E_INVALID, E_NOWEIGHTS = 0, -1, -6
TURN_LIMIT = 100000                                     # RO_TURN_LIMIT, csrc/bg_rollout.h
CHUNK = 131072                                          # the search's scratch env: at most this many lanes
FIELDS = ("rc", "P", "T", "N", "M", "rotate", "vr", "cube", "grouped", "two_ply", "slot", "run_flags", "F", "n_fan", "L", "fan_chunks",
          "fan_eval", "lane_offset", "R", "G", "truncates", "search_scratch_lanes", "preroll_positions", "preroll_lanes", "pos", "fan",
          "trials", "lanes", "vtrials", "vlanes", "vpos", "group", "ctrials", "cstart", "stall_turns", "stall_limit")


def refusal(q):
    """the code of a request that is refused before anything is issued, in the entry point's order, or OK"""
    flags, P, offset, T, M, lanes, has_states, has_group, plies, top_k, cube, w0, w1 = q
    if not has_states or P < 1 or T < 1 or M < 0 or lanes < 0 or offset < 0:
        return E_INVALID
    if flags & ~(ROTATE | SLOT1 | VR):
        return E_INVALID
    if P >= 2 ** 31 or T >= 2 ** 31 or P * T >= 2 ** 31 or lanes > 2 ** 30:
        return E_INVALID
    if cube and not flags & VR:
        return E_INVALID
    if not (w1 if flags & SLOT1 else w0):
        return E_NOWEIGHTS
    return OK


def scratch_lanes(n_virtual):
    """lanes of the search's scratch env for n_virtual virtual lanes: rounded up to 256, at most CHUNK"""
    return min(CHUNK, 256 * -(-n_virtual // 256))


def run_length(M, rotate, two_ply, divisor_descent=True):
    if two_ply:
        return 1
    if M == 0:
        return 8
    D = M - rotate
    if D < 1:
        return 1
    if not divisor_descent:                             # (a deliberately wrong reference)
        return min(D, 8)
    return [r for r in range(8, 0, -1) if D % r == 0][0]


def plan(q, divisor_descent=True, fan_by_trials=True, preroll_by_positions=True):
    """-> {field: int} of an accepted request, {"rc": code} of a refused one.  The three keywords switch on the deliberately wrong
    references of test_a_wrong_reference_fails_the_comparison."""
    rc = refusal(q)
    if rc:
        return {"rc": rc}
    flags, P, offset, T, M, lanes, has_states, has_group, plies, top_k, cube, w0, w1 = q
    rotate, vr, two_ply = int(bool(flags & ROTATE)), int(bool(flags & VR)), int(plies == 2)
    N = P * T
    F = (min(T, 36) if fan_by_trials else 36) if rotate else 0
    L = lanes if lanes > 0 else min(65536, 256 * -(-N // 256))
    R = run_length(M, rotate, two_ply, divisor_descent)
    G = 1 if R >= 16 else 16 // R
    pre = 0 if not vr else (max(P, L) if rotate and preroll_by_positions else L)
    return dict(rc=0, P=P, T=T, N=N, M=M, rotate=rotate, vr=vr, cube=int(bool(cube)), grouped=int(bool(has_group)), two_ply=two_ply,
                slot=int(bool(flags & SLOT1)), run_flags=flags & SLOT1, F=F, n_fan=P * F, L=L, fan_chunks=-(-(P * F) // L),
                fan_eval=int(rotate and M == 1), lane_offset=(offset * T - L) % 2 ** 64, R=R, G=G, truncates=int(M > 0),
                search_scratch_lanes=scratch_lanes(L * (top_k if top_k > 0 else 8) * 21) if two_ply else 0,
                preroll_positions=pre, preroll_lanes=scratch_lanes(pre * 21) if vr else 0,
                pos=P, fan=P * F, trials=N, lanes=L, vtrials=N * vr, vlanes=L * vr, vpos=P * vr, group=P if has_group else 0,
                ctrials=N if cube else 0, cstart=P if cube else 0, stall_turns=G * R, stall_limit=TURN_LIMIT + 64)


def render(d):
    """a plan as the driver prints it"""
    return "rc %d" % d["rc"] if d["rc"] else " ".join("%s %d" % (k, d[k]) for k in FIELDS)


def progress(N, R, G, reads):
    """The loop's verdict on each read-back (done, ro_err, env_err) in order: 0 go on, 1 finished, 2 stalled.  The loop as it stood:
    finished when every trial is done or either error word is set; else G R turns were issued since the read before, and they count as
    stalled when the done counter has not moved (it starts at 0); more than TURN_LIMIT + 64 stalled turns: give up."""
    out, last, stalled = [], 0, 0
    for done, ro_err, env_err in reads:
        if done >= N or ro_err or env_err:
            out.append(1)
            continue
        stalled = stalled + G * R if done == last else 0
        last = done
        out.append(2 if stalled > TURN_LIMIT + 64 else 0)
    return out
