"""The cut of a run-ahead pass of mrca_step_many into ray-cast launches, restated in Python: what test_gpu_multitick_raycast.py
proves its premise with, and what test_pass_plan_host.py holds csrc/mrca_pass_plan.h to."""

PASS_TICKS = 256          # csrc/mrca_pass_plan.h kAheadTicks (the envs of these tests are small: the ring has a slot per tick of a pass)


def launch_plan(K, T):
    """(first tick, ticks) of every ray-cast launch of a world range in a run-ahead pass of K ticks at T ticks per launch:
    plan_pass's cut (csrc/mrca_pass_plan.h) -- blocks [0], [1], two, four times T (T = 2: once), then 2 T each, a block in
    launches of up to T ticks, and an odd number of launches of several ticks made even by sending the first of them tick by
    tick."""
    blocks, a = [], 0
    while a < K:
        nb = len(blocks)
        n = (1 if a < 4 else 4) if T == 1 else (1 if nb < 2 else 2 if nb == 2 else T if nb < (7 if T > 2 else 4) else 2 * T)
        blocks.append((a, min(K, a + n)))
        a += n
    launches = []
    for a, e in blocks:
        for k in range(a, e, T):
            launches.append((k, min(T, e - k)))
    if sum(n > 1 for _k, n in launches) % 2:
        i = next(i for i, (_k, n) in enumerate(launches) if n > 1)
        k, n = launches[i]
        launches[i:i + 1] = [(k + q, 1) for q in range(n)]
    return launches
