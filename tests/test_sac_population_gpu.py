"""NativeSACPopulation (sacenv_sac_pop.hip, include/sacenv_population.h) against P separate
NativeSAC agents, bit for bit.

A population launch runs the device code of the one-agent kernels on the same f32 scalars
(sacenv_sac.hip: member_scalars), learn() has no atomics and every reduction has a fixed order,
so member m of a population must end with exactly the bytes agent m ends with: ``torch.equal``
on the whole slab (parameters, both Adam moments, the kernel copies of the 256x256 layers, the
target net) and on the losses. The first test checks the premise -- two equal agents given the
same batch end equal -- and the others mean nothing without it.

Inputs are generated as tests/test_sac_native_gpu.py::_batch generates them, per member with its
own seed. Shapes: batches 256, 512 and 768 cover the loop structures of the update launch
(small_chunk<8> / <4> tails, fc2 chunks of 12 and 4 k-blocks); P = 9 crosses the 8-XCD
round-robin; P = 1 is the degenerate case (sacenv_sac_pop_learn runs a one-member population on
the one-agent kernels, with member 0's values: the case checks that branch; the act launch has
no such branch).
"""
import ctypes as C
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

CANARY = 12345.0


def _cfg(m, B, max_size=1 << 14):
    """Member m's config: all five per-member values differ between members."""
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
    e1, e2 = torch.randn((B, 1), generator=g), torch.randn((B, 1), generator=g)
    dev = lambda x: x.to(gpu)  # noqa: E731
    return tuple(map(dev, (s, a, r, s2, d))), (dev(e1), dev(e2))


def _stacked(gpu, P, B, D, seed):
    """(per-member batches and noises, the same stacked [P, ...])."""
    per = [_batch(gpu, B, D, 1000 * seed + m) for m in range(P)]
    batch = tuple(torch.stack([per[m][0][k] for m in range(P)]) for k in range(5))
    noise = tuple(torch.stack([per[m][1][k] for m in range(P)]) for k in range(2))
    return per, batch, noise


def _agents(gpu, P, B, D, **kw):
    from sacenv.sac_native import NativeSAC
    return [NativeSAC(gpu, _cfg(m, B), obs_dim=D, init_seed=10 + m, with_memory=False, **kw) for m in range(P)]


def _population(gpu, P, B, D, **kw):
    from sacenv.population import NativeSACPopulation
    kw.setdefault("with_memory", False)
    return NativeSACPopulation(gpu, [_cfg(m, B) for m in range(P)], obs_dim=D,
                               init_seeds=[10 + m for m in range(P)], **kw)


def _same(pop, agents):
    torch.cuda.synchronize()
    for m, a in enumerate(agents):
        assert pop.weights[m].numel() == a.weights.numel()
        assert torch.equal(pop.weights[m], a.weights), f"member {m}: slab differs"
        # bitwise: the same f32 words (a NaN loss would still have to be the same NaN)
        assert torch.equal(pop.losses[m].view(torch.int32), a.losses.view(torch.int32)), f"member {m}: losses"


def test_two_equal_agents_learn_equal(gpu, built_lib):
    """The premise: one agent's learn() is the same from run to run, bit for bit."""
    from sacenv.sac_native import NativeSAC
    a, b = (NativeSAC(gpu, _cfg(1, 256), init_seed=3, with_memory=False) for _ in range(2))
    assert torch.equal(a.weights, b.weights)
    for k in range(3):
        batch, noise = _batch(gpu, 256, 11, 50 + k)
        a.learn(batch, noise, losses=False)
        b.learn(batch, noise, losses=False)
    torch.cuda.synchronize()
    assert torch.equal(a.weights, b.weights)
    assert torch.equal(a.losses, b.losses)


@pytest.mark.parametrize("P,B,D,kw", [
    (1, 256, 11, {}), (3, 256, 11, {}), (2, 768, 14, {}), (5, 512, 1, {}), (9, 256, 11, {}),
    (2, 256, 11, dict(max_action=0.5, adam_eps=1e-3))])
def test_population_learn_equals_separate_agents(gpu, built_lib, P, B, D, kw):
    agents = _agents(gpu, P, B, D, **kw)
    pop = _population(gpu, P, B, D, **kw)
    assert pop.weights.shape == (P, agents[0].weights.numel())
    for m, a in enumerate(agents):      # same initial weights and kernel copies (sync)
        assert torch.equal(pop.weights[m], a.weights), m
    for k in range(3):
        per, batch, noise = _stacked(gpu, P, B, D, k + 1)
        for m, a in enumerate(agents):
            a.learn(per[m][0], per[m][1], losses=False)
        out = pop.learn(batch, noise, losses=False)
        assert out is pop.losses and pop.adam_step == k + 1
        if k in (0, 2):
            _same(pop, agents)
    got = pop.learn(*_stacked(gpu, P, B, D, 9)[1:])     # losses=True: an independent [P, 4] copy
    assert got.shape == (P, 4) and got.data_ptr() != pop.losses.data_ptr() and torch.equal(got, pop.losses)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_population_act_equals_separate_acts(gpu, built_lib, n):
    """sacenv_sac_pop_act with a log-prob buffer against sacenv_sac_act per member. The outputs are
    [P][n], contiguous, between two 256-float canaries and padded with the canary to a multiple
    of 256: a member that wrote past its n rows would change the next member's rows or the pad."""
    from sacenv import _lib
    P, D = 3, 11
    pop = _population(gpu, P, 256, D)
    agents = [pop.export_member(m) for m in range(P)]
    g = torch.Generator().manual_seed(n)
    obs = (torch.rand((P, n, D), generator=g) * 1.2 - 0.1).to(gpu)
    eps = torch.randn((P, n), generator=g).to(gpu)
    tot = 256 + (P * n + 255) // 256 * 256 + 256
    act = torch.full((tot,), CANARY, device=gpu)
    lp = torch.full((tot,), CANARY, device=gpu)
    stream = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    _lib.check(built_lib.sacenv_sac_pop_act(C.byref(pop.params), P, pop.weights.data_ptr(), obs.data_ptr(), n,
                                            eps.data_ptr(), act[256:].data_ptr(), lp[256:].data_ptr(), stream))
    for m, a in enumerate(agents):
        wa, wl = torch.empty(n, device=gpu), torch.empty(n, device=gpu)
        _lib.check(built_lib.sacenv_sac_act(C.byref(a.params), a.weights.data_ptr(), obs[m].data_ptr(), n,
                                            eps[m].data_ptr(), wa.data_ptr(), wl.data_ptr(), stream))
        torch.cuda.synchronize()
        sl = slice(256 + m * n, 256 + (m + 1) * n)
        assert torch.equal(act[sl], wa), m
        assert torch.equal(lp[sl], wl), m
    for buf in (act, lp):
        assert bool((buf[:256] == CANARY).all()) and bool((buf[256 + P * n:] == CANARY).all())
    # the class's own call: the same actions, as [P, n, 1]
    out = pop.choose_action(obs, eps)
    assert out.shape == (P, n, 1) and torch.equal(out.reshape(-1), act[256: 256 + P * n])


def test_population_calls_touch_nothing_outside_their_buffers(gpu, built_lib):
    """weights, scratch and losses inside larger tensors with canaries on both sides: sync, act and
    learn leave every canary as it was."""
    from sacenv import _lib
    P, B, D, PAD = 3, 256, 11, 1024
    pop = _population(gpu, P, B, D)
    PL = pop.pop_layout
    sizes = dict(weights=PL.total_floats, scratch=PL.total_scratch_bytes // 4, losses=4 * P)
    big = {k: torch.full((n + 2 * PAD,), CANARY, device=gpu) for k, n in sizes.items()}
    inner = {k: big[k][PAD: PAD + n] for k, n in sizes.items()}
    inner["weights"].copy_(pop.weights.reshape(-1))
    _, batch, noise = _stacked(gpu, P, B, D, 4)
    s, a, r, s2, d = batch
    a, e1, e2 = (t.reshape(P, B).contiguous() for t in (a, noise[0], noise[1]))
    d = d.to(torch.uint8)
    n = 100
    obs, eps = s[:, :n].contiguous(), e1[:, :n].contiguous()
    out = torch.full((P * n + 2 * PAD,), CANARY, device=gpu)
    stream = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    pp, W = C.byref(pop.params), inner["weights"].data_ptr()
    _lib.check(built_lib.sacenv_sac_pop_sync(pp, P, W, stream))
    _lib.check(built_lib.sacenv_sac_pop_act(pp, P, W, obs.data_ptr(), n, eps.data_ptr(), out[PAD:].data_ptr(),
                                            None, stream))
    _lib.check(built_lib.sacenv_sac_pop_learn(pp, P, pop._hp, W, inner["scratch"].data_ptr(), s.data_ptr(),
                                              a.data_ptr(), r.data_ptr(), s2.data_ptr(), d.data_ptr(),
                                              e1.data_ptr(), e2.data_ptr(), 1, inner["losses"].data_ptr(), stream))
    pop.learn(batch, noise, losses=False)
    torch.cuda.synchronize()
    for k, n_in in sizes.items():
        assert bool((big[k][:PAD] == CANARY).all()), f"{k}: written before the buffer"
        assert bool((big[k][PAD + n_in:] == CANARY).all()), f"{k}: written past the buffer"
    assert bool((out[:PAD] == CANARY).all()) and bool((out[PAD + P * n:] == CANARY).all())
    assert not bool((out[PAD: PAD + P * n] == CANARY).any())
    # and the call on the framed buffers computed what the population's own buffers hold
    assert torch.equal(inner["weights"], pop.weights.reshape(-1))
    assert torch.equal(inner["losses"], pop.losses.reshape(-1))


def test_export_member_and_from_agents_round_trip(gpu, built_lib):
    from sacenv.population import NativeSACPopulation
    P, B, D = 3, 256, 11
    pop = _population(gpu, P, B, D)
    per, batch, noise = _stacked(gpu, P, B, D, 1)
    pop.learn(batch, noise, losses=False)
    copies = [pop.export_member(m) for m in range(P)]
    assert all(c.adam_step == 1 and c.cfg == pop.configs[m] for m, c in enumerate(copies))
    per, batch, noise = _stacked(gpu, P, B, D, 2)
    for m, c in enumerate(copies):      # a copy: its learn() leaves the population alone
        before = pop.weights[m].clone()
        c.learn(per[m][0], per[m][1], losses=False)
        assert torch.equal(pop.weights[m], before)
    pop.learn(batch, noise, losses=False)
    _same(pop, copies)
    # the reverse: a population from agents that have learned once
    agents = _agents(gpu, P, B, D)
    per, batch, noise = _stacked(gpu, P, B, D, 3)
    for m, a in enumerate(agents):
        a.learn(per[m][0], per[m][1], losses=False)
    back = NativeSACPopulation.from_agents(agents)
    assert back.adam_step == 1 and back.memory is None
    torch.cuda.synchronize()
    for m, a in enumerate(agents):
        assert torch.equal(back.weights[m], a.weights), m
    per, batch, noise = _stacked(gpu, P, B, D, 4)
    for m, a in enumerate(agents):
        a.learn(per[m][0], per[m][1], losses=False)
    back.learn(batch, noise, losses=False)
    _same(back, agents)
    # agents that differ in a shared field or in their step are refused
    agents[1].adam_step += 1
    with pytest.raises(ValueError, match="step"):
        NativeSACPopulation.from_agents(agents)
    agents[1].adam_step -= 1
    other = _agents(gpu, 1, 512, D)[0]
    with pytest.raises(ValueError):
        NativeSACPopulation.from_agents([agents[0], other])
    # out and in again, with noise seeds and an act count: weights, step, act count and seeds come back
    for P in (1, 3):
        seeds = tuple(2 ** 63 + 5 - m for m in range(P))
        pop = _population(gpu, P, B, D, noise_seeds=seeds)
        per, batch, noise = _stacked(gpu, P, B, D, 5)
        pop.choose_action(batch[0][:, :65])
        pop.learn(batch, noise, losses=False)
        copies = [pop.export_member(m) for m in range(P)]
        for m, c in enumerate(copies):
            assert (c.adam_step, c.act_calls, c.noise_seed, c.memory) == (1, 1, seeds[m], None)
            assert c.cfg == pop.configs[m] and c.params.adam_eps == pop.params.adam_eps
            assert c.weights.data_ptr() != pop.weights[m].data_ptr() and torch.equal(c.weights, pop.weights[m])
        back = NativeSACPopulation.from_agents(copies)
        assert (back.adam_step, back.act_calls, back.noise_seeds, back.configs) == (1, 1, seeds, pop.configs)
        assert torch.equal(back.weights, pop.weights)
        obs = batch[0][:, :63]
        assert torch.equal(back.choose_action(obs), pop.choose_action(obs))      # the seeded draw of act 1
        _, batch, _ = _stacked(gpu, P, B, D, 6)
        back.learn(batch, losses=False)                                         # and of step 1
        pop.learn(batch, losses=False)
        torch.cuda.synchronize()
        assert torch.equal(back.weights, pop.weights) and torch.equal(back.losses, pop.losses)


@pytest.mark.parametrize("optimizer", [False, True])
def test_save_and_load_models_per_member(gpu, built_lib, tmp_path, optimizer):
    import os
    from sacenv.agent import CHECKPOINT_NAMES
    P, B, D = 2, 256, 11
    pop = _population(gpu, P, B, D)
    _, batch, noise = _stacked(gpu, P, B, D, 1)
    pop.learn(batch, noise, losses=False)
    pop.save_models(str(tmp_path), optimizer=optimizer)
    for m in range(P):
        for f in CHECKPOINT_NAMES.values():
            assert os.path.exists(tmp_path / f"member_{m}" / "checkpoints" / f)
    from sacenv.population import NativeSACPopulation
    fresh = NativeSACPopulation(gpu, pop.configs, obs_dim=D, init_seeds=[77, 78], with_memory=False)
    assert not torch.equal(fresh.weights, pop.weights)
    fresh.load_models(str(tmp_path), optimizer=optimizer)
    torch.cuda.synchronize()
    L = pop.layout
    n_params = L.adam_m[0]              # the five nets come first in a slab
    assert torch.equal(fresh.weights[:, :n_params], pop.weights[:, :n_params])
    assert torch.equal(fresh.weights[:, L.w2f[0]:], pop.weights[:, L.w2f[0]:])      # the kernel copies (sync)
    if optimizer:                       # the moments and the step too: the next learn() is the same
        assert fresh.adam_step == pop.adam_step == 1
        assert torch.equal(fresh.weights, pop.weights)
        _, batch, noise = _stacked(gpu, P, B, D, 2)
        pop.learn(batch, noise, losses=False)
        fresh.learn(batch, noise, losses=False)
        torch.cuda.synchronize()
        assert torch.equal(fresh.weights, pop.weights) and torch.equal(fresh.losses, pop.losses)
    else:
        assert fresh.adam_step == 0


def test_host_write_and_sync_reach_the_next_act(gpu, built_lib):
    P, D, n = 2, 11, 130
    pop = _population(gpu, P, 256, D)
    g = torch.Generator().manual_seed(8)
    obs = (torch.rand((P, n, D), generator=g) * 1.2 - 0.1).to(gpu)
    eps = torch.randn((P, n), generator=g).to(gpu)
    before = pop.choose_action(obs, eps)
    with torch.no_grad():
        pop.members[1].actor.fc2.weight.mul_(0.5)
    stale = pop.choose_action(obs, eps)
    assert torch.equal(stale, before)           # the kernels read their own copy of fc2.weight
    donor = pop.export_member(1)                # one agent with the written weights, synced on its own
    donor.sync()
    pop.sync()
    after = pop.choose_action(obs, eps)
    torch.cuda.synchronize()
    assert torch.equal(after[0], before[0])     # member 0 was not written
    assert not torch.equal(after[1], before[1])
    assert torch.equal(after[1], donor.choose_action(obs[1], eps[1]))


def test_population_learns_from_its_members_buffers(gpu, built_lib):
    P, B, D = 2, 256, 11
    seeds = [5, 6]
    pops = [_population(gpu, P, B, D, with_memory=True, buffer_seeds=seeds) for _ in range(2)]
    noise = _stacked(gpu, P, B, D, 7)[2]

    def store(m, n, seed):
        (s, a, r, s2, d), _ = _batch(gpu, n, D, seed)
        for pop in pops:
            pop.remember(m, s, a, r.to(torch.float32), s2, d.to(torch.uint8))

    assert pops[0].learn(noise=noise) is None                   # nothing stored
    store(0, 300, 1)
    store(1, 200, 2)
    assert pops[0].learn(noise=noise) is None                   # member 1 holds 200 < B rows
    assert pops[0].adam_step == 0
    store(1, 100, 3)
    assert [mem.mem_cntr for mem in pops[0].memory] == [300, 300]
    got = pops[0].learn(noise=noise)
    assert got is not None and got.shape == (P, 4) and pops[0].adam_step == 1
    # the same rows through the explicit path: the other population's samplers, same seeds
    rows = [mem.sample(B, as_bool=False)[:5] for mem in pops[1].memory]
    assert not torch.equal(rows[0][0], rows[1][0])
    batch = tuple(torch.stack([r[k] for r in rows]) for k in range(5))
    want = pops[1].learn(batch, noise)
    torch.cuda.synchronize()
    assert torch.equal(pops[0].weights, pops[1].weights)
    assert torch.equal(got, want)


def test_bad_shapes_raise_before_any_launch(gpu, built_lib):
    from sacenv import _lib
    P, B, D = 2, 256, 11
    pop = _population(gpu, P, B, D)
    w0 = pop.weights.clone()
    _, batch, noise = _stacked(gpu, P, B, D, 1)
    _, batch3, noise3 = _stacked(gpu, 3, B, D, 1)
    with pytest.raises(ValueError):
        pop.learn(batch3, noise3)                               # a wrong P
    with pytest.raises(ValueError):
        pop.learn(batch, noise3)
    with pytest.raises(ValueError):
        pop.learn(tuple(t[:, : B // 2] for t in batch), noise)  # half a batch
    for k in range(5):
        bad = list(batch)
        bad[k] = bad[k][:1]
        with pytest.raises(ValueError):
            pop.learn(tuple(bad), noise)
    with pytest.raises(ValueError):
        pop.choose_action(batch3[0])
    with pytest.raises(ValueError):
        pop.choose_action(batch[0][0])                          # [n, D]: no member axis
    with pytest.raises(ValueError):
        pop.choose_action(batch[0], noise3[0])
    with pytest.raises((ValueError, _lib.SacenvError)):         # one member too many for the kernels' table
        _population(gpu, _lib.POPULATION_MAX_MEMBERS + 1, B, D)
    torch.cuda.synchronize()
    assert pop.adam_step == 0 and torch.equal(pop.weights, w0)
    assert dataclasses.is_dataclass(pop.configs[0])


def test_refused_calls_change_nothing(gpu, built_lib):
    """Every ``ValueError`` case of ``test_bad_shapes_raise_before_any_launch`` is a host-side
    refusal: the step, the act count, the weights and the losses stay bit for bit, and the next good
    ``learn`` is the one of a population that never saw them."""
    from sacenv import _lib
    from test_sac_native_gpu import _bits, same_bits
    P, B, D = 2, 256, 11
    pop, twin = (_population(gpu, P, B, D) for _ in range(2))
    _, batch, noise = _stacked(gpu, P, B, D, 1)
    _, batch3, noise3 = _stacked(gpu, 3, B, D, 1)
    for p in (pop, twin):           # one accepted act and learn first: non-trivial counters, moments and losses
        p.choose_action(batch[0][:, :65], noise[0][:, :65])
        p.learn(batch, noise, losses=False)
    before = _bits(pop)
    assert before[:2] == (1, 1)
    bad = [lambda: pop.learn(batch3, noise3), lambda: pop.learn(batch, noise3),
           lambda: pop.learn(tuple(t[:, : B // 2] for t in batch), noise),
           lambda: pop.choose_action(batch3[0]), lambda: pop.choose_action(batch[0][0]),
           lambda: pop.choose_action(batch[0], noise3[0]),
           lambda: _population(gpu, _lib.POPULATION_MAX_MEMBERS + 1, B, D)]
    for k in range(5):
        cut = list(batch)
        cut[k] = cut[k][:1]
        bad.append(lambda cut=tuple(cut): pop.learn(cut, noise))
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert same_bits(_bits(pop), before), i
    _, batch, noise = _stacked(gpu, P, B, D, 2)
    pop.learn(batch, noise, losses=False)
    twin.learn(batch, noise, losses=False)
    assert _bits(pop)[:2] == (2, 1) and same_bits(_bits(pop), _bits(twin))


@pytest.mark.parametrize("path", ["unseeded", "seeded", "from_agents", "export_member"])
def test_construction_leaves_the_generators_as_before(gpu, built_lib, path):
    """Per constructing path, the CPU net builds it makes (``from_agents`` and ``export_member``
    build unseeded nets they then overwrite) leave torch's generators as those builds alone do
    (tests/test_sac_native_gpu.py: ``check_generators``)."""
    from sacenv.population import NativeSACPopulation
    from test_sac_native_gpu import check_generators
    P, B, D = 2, 256, 11
    cfgs = [_cfg(m, B) for m in range(P)]
    if path in ("unseeded", "seeded"):
        seeds = [10, 11] if path == "seeded" else None
        made = check_generators(gpu, 31, lambda: NativeSACPopulation(gpu, cfgs, obs_dim=D, init_seeds=seeds,
                                                                     noise_seeds=[3, 4]), cfgs, seeds, D)
    elif path == "from_agents":
        agents = _agents(gpu, P, B, D, noise_seed=3)
        made = check_generators(gpu, 31, lambda: NativeSACPopulation.from_agents(agents), cfgs, None, D)
    else:
        pop = _population(gpu, P, B, D, noise_seeds=[3, 4])
        made = check_generators(gpu, 31, lambda: pop.export_member(1), cfgs[1:], None, D)
    assert made is not None
