"""Counter-based policy noise on the device (sacenv_noise.hip, include/sacenv_noise.h,
sacenv/noise.py) and the agents that draw from it.

The kernel is held to the contract's exact values (tests/noise_oracle.py: mpmath at 120 bits,
rounded once to f32) within 1 f32 ulp. That bound is derived, not measured: the device evaluates
the contract in f64, where log, sqrt, sincospi (exact argument reduction) and one multiply leave
a relative error of a few 2^-53, far under the 2^-30 below which the one rounding to f32 lands
on the exact value's f32 or its neighbour. Where the exact value is 0 the device's is 0.

Everything else is bit-exact (``torch.equal``): the draws do not depend on how they are grouped
into launches, members or calls; a seeded agent equals an agent given the same noise explicitly;
member m of a seeded population equals a stand-alone seeded ``NativeSAC``; and the search loop of
examples/train_population.py, run for one member alone, reproduces that member's weights, replay
bytes and losses (the test that needs the feature: torch's one stream cannot give it).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import noise_oracle as no

pytestmark = pytest.mark.gpu

SEEDS4 = (0, 1, 2 ** 32 - 1, 2 ** 63 + 5)
BOAT = {"base_settings": {"experiment": 6, "test_mode": 0}}


def _noise(gpu, seeds):
    from sacenv.noise import PolicyNoise
    return PolicyNoise(seeds, gpu)


def _check_rows(got, seeds, stream, first_call, oracle):
    """got [calls, P, n] against the oracle row by row: (worst ulp, values not bit-equal)."""
    got = got.cpu().numpy()
    calls, P, n = got.shape
    worst = differing = 0
    for k in range(calls):
        for m in range(P):
            want = oracle(seeds[m], stream, first_call + k, n)
            d = no.ulp_distance(got[k, m], want)
            worst, differing = max(worst, int(d.max())), differing + int((d != 0).sum())
            assert not got[k, m][want == 0].any(), (k, m)
    assert np.isfinite(got).all() and np.abs(got).max() < no.BOUND
    return worst, differing


def test_parity_with_the_exact_values(gpu, built_lib):
    """One call, four members, three draws; every value within 1 f32 ulp of mpmath's."""
    noise = _noise(gpu, SEEDS4)
    reqs = [(0, 0, 5, 1), (1, 2 ** 31, 64, 3), (2, 2 ** 40, 257, 2)]
    outs = noise.draw(reqs)
    worst = differing = total = 0
    for (stream, first, n, calls), got in zip(reqs, outs):
        assert got.shape == (calls, 4, n) and got.dtype == torch.float32
        w, d = _check_rows(got, SEEDS4, stream, first, no.normal_mp)
        worst, differing, total = max(worst, w), differing + d, total + got.numel()
    print(f"device vs mpmath on {total} values: worst {worst} f32 ulp, {differing} not bit-equal")
    assert worst <= 1


def test_parity_with_the_numpy_restatement(gpu, built_lib):
    """n = 4 099 (1 025 Philox blocks: 17 workgroups per row, a partial last block), calls = 2."""
    noise = _noise(gpu, SEEDS4)
    got = noise.normal(1, 7, 4099, calls=2)
    worst, differing = _check_rows(got, SEEDS4, 1, 7, no.normal_np)
    print(f"device vs numpy on {got.numel()} values: worst {worst} f32 ulp, {differing} not bit-equal")
    assert worst <= 1


def test_the_draws_do_not_depend_on_their_grouping(gpu, built_lib):
    seeds = (11, 2 ** 63 + 5, 3, 2 ** 32 - 1, 77)
    five = _noise(gpu, seeds)
    # a member alone = its row among five
    big = five.normal(0, 9, 200)
    for m, s in enumerate(seeds):
        assert torch.equal(_noise(gpu, [s]).normal(0, 9, 200)[0, 0], big[0, m]), m
    assert torch.equal(_noise(gpu, [seeds[1], seeds[4]]).normal(0, 9, 200)[0], big[0, [1, 4]])
    # three draws in one call = three calls of one draw
    reqs = [(0, 4, 65, 1), (1, 2, 256, 2), (2, 2, 256, 1)]
    for a, r in zip(five.draw(reqs), reqs):
        assert torch.equal(a, five.normal(*r))
    # row k of a table = the single call first_call + k
    table = five.normal(0, 2 ** 31 - 2, 130, calls=4)
    for k in range(4):
        assert torch.equal(table[k], five.normal(0, 2 ** 31 - 2 + k, 130)[0]), k
    # prefix property
    assert torch.equal(five.normal(2, 5, 63), five.normal(2, 5, 200)[:, :, :63])
    # streams, calls and seeds apart
    base = five.normal(0, 9, 200)[0]
    assert not torch.equal(base, five.normal(1, 9, 200)[0]) and not torch.equal(base, five.normal(0, 10, 200)[0])
    assert len({tuple(row.tolist()) for row in base}) == 5


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025])
def test_nothing_is_written_outside_the_outputs(gpu, built_lib, n):
    """Two draws of one launch, each inside its own window of 0xA5 bytes at an offset that is
    only 4-B aligned; the bytes around them stay, and the values are the class's."""
    from sacenv import _lib
    P, calls, PAD = 3, 2, 1028
    noise = _noise(gpu, (5, 6, 7))
    size = 4 * calls * P * n
    buf = torch.full((2 * (PAD + size + PAD),), 0xA5, dtype=torch.uint8, device=gpu)
    starts = (PAD, PAD + size + PAD + PAD)
    assert buf.data_ptr() % 16 == 0 and all(s % 8 == 4 for s in starts)
    desc = (_lib.NoiseDraw * 2)()
    for d, start, (stream, first) in zip(desc, starts, ((0, 3), (2, 2 ** 33))):
        d.stream, d.first_call, d.calls, d.n, d.out = stream, first, calls, n, buf.data_ptr() + start
    seeds = (C.c_uint64 * P)(5, 6, 7)
    stream_h = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    assert built_lib.sacenv_noise_normal(P, seeds, 2, desc, stream_h) == 0
    torch.cuda.synchronize()
    inside = torch.zeros_like(buf, dtype=torch.bool)
    for start, (stream, first) in zip(starts, ((0, 3), (2, 2 ** 33))):
        inside[start: start + size] = True
        got = buf[start: start + size].clone().view(torch.float32).view(calls, P, n)
        assert torch.equal(got, noise.normal(stream, first, n, calls=calls))
    assert bool((buf[~inside] == 0xA5).all())
    # an empty draw beside a full one writes nothing of its own
    buf.fill_(0xA5)
    desc[0].n = 0
    desc[0].out = None
    assert built_lib.sacenv_noise_normal(P, seeds, 2, desc, stream_h) == 0
    torch.cuda.synchronize()
    inside[starts[0]: starts[0] + size] = False
    assert bool((buf[~inside] == 0xA5).all()) and not bool((buf[inside] == 0xA5).all())


def _cfg(m, B=256, max_size=1 << 12):
    from sacenv.agent import AgentConfig
    return AgentConfig(lr_alpha=0.0015 + 0.001 * m, lr_beta=0.0003 * (m + 2), gamma=0.95 + 0.004 * m,
                       tau=0.002 * (m + 1), reward_scale=2.0 + m, batch_size=B, max_size=max_size)


def _batch(gpu, B, D, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.rand((B, D), generator=g) * 1.2 - 0.1
    a = torch.rand((B, 1), generator=g) * 2 - 1
    r = (torch.rand(B, generator=g, dtype=torch.float64) - 0.8) * 3
    s2 = s + 0.01 * torch.randn((B, D), generator=g)
    d = torch.rand(B, generator=g) < 0.1
    return tuple(x.to(gpu) for x in (s, a, r, s2, d))


def _obs(gpu, shape, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 1.2 - 0.1).to(gpu)


def test_seeded_agent_equals_explicit_noise(gpu, built_lib):
    from sacenv.noise import ACT, LEARN1, LEARN2
    from sacenv.sac_native import NativeSAC
    seed, B, D, n = 2 ** 63 + 5, 256, 11, 65
    a = NativeSAC(gpu, _cfg(1), init_seed=3, with_memory=False, noise_seed=seed)
    b = NativeSAC(gpu, _cfg(1), init_seed=3, with_memory=False)
    noise = _noise(gpu, [seed])
    assert a.noise_seed == seed and b.noise_seed is None and b.noise is None
    assert "act_calls" in a.optimizer_state() and "act_calls" not in b.optimizer_state()
    for call in range(3):
        obs = _obs(gpu, (n, D), call)
        assert a.act_calls == call
        want = b.choose_action(obs, eps=noise.normal(ACT, call, n)[0, 0])
        assert torch.equal(a.choose_action(obs), want), call
    assert a.act_calls == 3
    a.choose_action(_obs(gpu, (n, D), 9), eps=torch.zeros(n, device=gpu))     # an explicit eps counts too
    assert a.act_calls == 4
    with pytest.raises(ValueError):
        a.choose_action(_obs(gpu, (n, D + 1), 9))                             # refused: no act counted
    assert a.act_calls == 4
    for step in range(2):
        batch = _batch(gpu, B, D, 40 + step)
        assert a.adam_step == step
        e1, e2 = noise.draw([(LEARN1, step, B), (LEARN2, step, B)])
        la = a.learn(batch)
        lb = b.learn(batch, noise=(e1[0, 0], e2[0, 0]))
        assert all(torch.equal(x, y) for x, y in zip(la, lb)), step
    torch.cuda.synchronize()
    assert torch.equal(a.weights, b.weights) and a.adam_step == b.adam_step == 2
    # explicit noise still wins on a seeded agent, and noise_for_step is those draws without a state change
    eps, (e1, e2) = a.noise_for_step(n)
    assert (a.act_calls, a.adam_step) == (4, 2)
    assert torch.equal(eps, noise.normal(ACT, 4, n)[0, 0])
    assert torch.equal(e1, noise.normal(LEARN1, 2, B)[0, 0]) and torch.equal(e2, noise.normal(LEARN2, 2, B)[0, 0])
    batch = _batch(gpu, B, D, 50)
    z = (torch.zeros(B, device=gpu), torch.ones(B, device=gpu))
    a.learn(batch, noise=z)
    b.learn(batch, noise=z)
    assert torch.equal(a.weights, b.weights)


def test_seeded_population_equals_stand_alone_agents(gpu, built_lib):
    from sacenv.population import NativeSACPopulation
    from sacenv.sac_native import NativeSAC
    P, B, D, n = 3, 256, 11, 65
    seeds = (7, 2 ** 32 - 1, 2 ** 63 + 5)
    pop = NativeSACPopulation(gpu, [_cfg(m) for m in range(P)], obs_dim=D, init_seeds=[10 + m for m in range(P)],
                              with_memory=False, noise_seeds=seeds)
    agents = [NativeSAC(gpu, _cfg(m), obs_dim=D, init_seed=10 + m, with_memory=False, noise_seed=seeds[m])
              for m in range(P)]
    for call in range(3):
        obs = _obs(gpu, (P, n, D), call)
        out = pop.choose_action(obs)
        for m, a in enumerate(agents):
            assert torch.equal(out[m], a.choose_action(obs[m])), (call, m)
    assert pop.act_calls == 3
    for step in range(2):
        per = [_batch(gpu, B, D, 100 * step + m) for m in range(P)]
        losses = pop.learn(tuple(torch.stack([per[m][k] for m in range(P)]) for k in range(5)))
        for m, a in enumerate(agents):
            a.learn(per[m], losses=False)
            assert torch.equal(losses[m].view(torch.int32), a.losses.view(torch.int32)), (step, m)
    torch.cuda.synchronize()
    for m, a in enumerate(agents):
        assert torch.equal(pop.weights[m], a.weights), m
    # members out and in carry the seed and the act count
    out1 = pop.export_member(1)
    assert (out1.noise_seed, out1.act_calls, out1.adam_step) == (seeds[1], 3, 2)
    back = NativeSACPopulation.from_agents(agents)
    assert back.noise_seeds == seeds and (back.act_calls, back.adam_step) == (3, 2)
    obs = _obs(gpu, (P, n, D), 77)
    assert torch.equal(back.choose_action(obs), pop.choose_action(obs))
    assert torch.equal(out1.choose_action(obs[1]), agents[1].choose_action(obs[1]))
    with pytest.raises(ValueError):
        NativeSACPopulation.from_agents([agents[0], out1])      # act counts 3 and 4
    with pytest.raises(ValueError):
        NativeSACPopulation(gpu, [_cfg(0), _cfg(1)], with_memory=False, noise_seeds=[1])


def test_the_search_loop_reproduces_one_member_alone(gpu, built_lib):
    """The loop of examples/train_population.py with P = 2, N = 64, batch 256 for 6 iterations
    (256 rows after iteration 4: iterations 4, 5 and 6 learn), then member 1 alone: a ``NativeSAC``
    with the same init, buffer and noise seeds, a ``DeviceReplayBuffer`` and the 64 envs with global
    ids 64..127. Member 1's weight slab, replay bytes and losses are the stand-alone run's."""
    from sacenv import NativeSACPopulation, PopulationReplay, VecBoatEnv
    from sacenv.sac_native import NativeSAC
    P, N, B, iters, M = 2, 64, 256, 6, 1 << 12
    cfgs = [_cfg(m, B, M) for m in range(P)]
    nseeds = (1234, 2 ** 63 + 5)
    torch.manual_seed(99)       # torch's stream plays no part: the second run starts it elsewhere
    replay = PopulationReplay(P, M, (11,), 1, device=gpu, seeds=[20, 21])
    pop = NativeSACPopulation(gpu, cfgs, init_seeds=[30, 31], replay=replay, noise_seeds=nseeds)
    env = VecBoatEnv(BOAT, P * N, seed=0, device=gpu, max_episode_steps=500)
    obs = env.reset().clone()
    pop_losses = []
    for _ in range(iters):
        eps, noise = pop.noise_for_step(N)
        a = pop.choose_action(obs.view(P, N, -1), eps=eps)
        env.step(a.view(-1))
        replay.store_env_step(obs, a, env)
        obs = env.obs.clone()
        out = pop.learn(noise=noise, losses=False)
        pop_losses.append(None if out is None else out[1].clone())
    assert [l is not None for l in pop_losses] == [False] * 3 + [True] * 3
    assert (pop.act_calls, pop.adam_step) == (6, 3)

    torch.manual_seed(5)
    torch.randn(1000, device=gpu)
    m = 1
    agent = NativeSAC(gpu, cfgs[m], init_seed=31, buffer_seed=21, noise_seed=nseeds[m])
    env1 = VecBoatEnv(BOAT, N, seed=0, device=gpu, max_episode_steps=500, env_id_offset=m * N)
    obs1 = env1.reset().clone()
    for it in range(iters):
        a = agent.choose_action(obs1)
        env1.step(a.view(-1))
        agent.memory.store_env_step(obs1, a, env1)
        obs1 = env1.obs.clone()
        out = agent.learn(losses=False)
        assert (out is None) == (pop_losses[it] is None), it
        if out is not None:
            assert torch.equal(out.view(torch.int32), pop_losses[it].view(torch.int32)), it
    torch.cuda.synchronize()
    assert torch.equal(obs1, obs[m * N: (m + 1) * N])
    assert pop.weights[m].numel() == agent.weights.numel() and torch.equal(pop.weights[m], agent.weights)
    assert torch.equal(replay.arena[m], agent.memory.arena)
    assert (agent.act_calls, agent.adam_step) == (6, 3)


def test_act_noise_closed_loop_and_checkpoints(gpu, built_lib, tmp_path):
    from sacenv import VecBoatEnv
    from sacenv.closed_loop import ClosedLoop
    from sacenv.noise import ACT
    from sacenv.population import NativeSACPopulation
    from sacenv.sac_native import NativeSAC
    K, N, B, D, seed = 5, 128, 256, 11, 42
    mk = lambda: NativeSAC(gpu, _cfg(0), init_seed=3, with_memory=False, noise_seed=seed)  # noqa: E731
    a, b = mk(), mk()
    a.choose_action(_obs(gpu, (N, D), 0))
    b.choose_action(_obs(gpu, (N, D), 0))
    # act_noise rows = the next K choose_action draws
    table = a.act_noise(K, N)
    assert table.shape == (K, N) and a.act_calls == 1
    noise = _noise(gpu, [seed])
    for k in range(K):
        assert torch.equal(table[k], noise.normal(ACT, 1 + k, N)[0, 0]), k
    pop = NativeSACPopulation(gpu, [_cfg(0), _cfg(1)], with_memory=False, noise_seeds=[seed, 9])
    pt = pop.act_noise(K, 65)
    assert pt.shape == (K, 2, 65) and torch.equal(pt[:, 0], noise.normal(ACT, 0, 65, calls=K)[:, 0])
    # ClosedLoop.run_eager(act_noise) = K seeded choose_action + step pairs
    kw = dict(seed=9, device=gpu, max_episode_steps=50)
    ea, eb = VecBoatEnv(BOAT, N, **kw), VecBoatEnv(BOAT, N, **kw)
    ea.reset()
    eb.reset()
    ClosedLoop(ea, a, segment=K).run_eager(table)
    for _ in range(K):
        eb.step_async(b.choose_action(eb.obs).view(-1))
    torch.cuda.synchronize()
    assert torch.equal(ea.arena, eb.arena) and a.act_calls == b.act_calls == 1 + K
    # a checkpoint with optimizer=True resumes the same next act and learn
    a.learn(_batch(gpu, B, D, 1))
    a.save_models(str(tmp_path), optimizer=True)
    c = mk()
    c.load_models(str(tmp_path), optimizer=True)
    assert (c.act_calls, c.adam_step) == (a.act_calls, a.adam_step) == (1 + K, 1)
    obs, batch = _obs(gpu, (N, D), 5), _batch(gpu, B, D, 2)
    assert torch.equal(c.choose_action(obs), a.choose_action(obs))
    la, lc = a.learn(batch), c.learn(batch)
    assert all(torch.equal(x, y) for x, y in zip(la, lc)) and torch.equal(a.weights, c.weights)
    # the population's checkpoints carry its one act count
    pop.choose_action(_obs(gpu, (2, 65, D), 1))
    pop.save_models(str(tmp_path / "pop"), optimizer=True)
    pop2 = NativeSACPopulation(gpu, [_cfg(0), _cfg(1)], with_memory=False, noise_seeds=[seed, 9])
    pop2.load_models(str(tmp_path / "pop"), optimizer=True)
    assert pop2.act_calls == pop.act_calls == 1
    obs = _obs(gpu, (2, 65, D), 2)
    assert torch.equal(pop2.choose_action(obs), pop.choose_action(obs))


def test_statistics_on_the_device(gpu, built_lib):
    x = _noise(gpu, [2]).normal(0, 1, 1 << 20)[0, 0].cpu().numpy()
    assert np.isfinite(x).all() and np.abs(x).max() < no.BOUND
    stats = no.statistics(x)
    name = max(stats, key=lambda k: abs(stats[k]))
    print(f"device, seed 2, stream 0, call 1: worst {stats[name]:+.2f} sigma ({name})")
    for k, v in stats.items():
        assert abs(v) <= 5.0, (k, v)
