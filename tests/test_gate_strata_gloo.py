"""
montecarlo.gate_strata_sharded for the two post-selected gadgets on the CPU: four torch.distributed (gloo) processes each draw their
shard of every stratum's sample range with the host statement (local_fn) and all-reduce the nstrata x 17 x F counts; every rank must
end with the one-rank SampledGateStrata.  tests/test_gadget_strata_gloo.py's pattern: what is under test is the sharding arithmetic,
the field count taken from the part, and the collective, which are the same code on RCCL.
"""
import os
import socket
import sys

import numpy as np
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 4
STRATA = [(0, 0), (1, 0), (2, 1), (0, 16)]
SAMPLES = [5, 2001, 4003, 778]                                # no multiple of four: the first ranks take the extra samples
FIRSTS = [0, 10, 10, 123456]
SEED = 20261019


def _gadgets():
    from oracle import cpu_ref
    from quantum_css_codes_amd import ec_noise, ft_noise
    h = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
    code = cpu_ref.CSSCode(h, h)
    return ec_noise.ECCircuit(code, 2), ft_noise.FTProgram(code, "X")


def _host(gadget, strata, samples, seed, first_sample):
    return gadget.gate_strata(strata, samples, seed=seed, first_sample=first_sample, host=True)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from quantum_css_codes_amd import montecarlo
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for name, gadget in zip(("ec", "ft"), _gadgets()):
        got = montecarlo.gate_strata_sharded(gadget, STRATA, SAMPLES, SEED, FIRSTS, local_fn=_host)
        assert isinstance(got, montecarlo.SampledGateStrata) and (got.n1, got.n2) == gadget.gate_sites()[1:3]
        assert got.samples.tolist() == SAMPLES and got.strata.tolist() == [list(s) for s in STRATA]
        out[name + "_fields"] = np.array(got.fields)
        out[name] = got.counts
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    dist.destroy_process_group()


def test_four_rank_gate_strata_equal_the_one_rank_strata(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(WORLD, port, str(tmp_path)), nprocs=WORLD, join=True)
    from quantum_css_codes_amd import ec_noise, ft_noise, montecarlo
    for name, gadget, fields in zip(("ec", "ft"), _gadgets(), (ec_noise.EC_FIELDS, ft_noise.FT_FIELDS)):
        whole = _host(gadget, STRATA, SAMPLES, SEED, FIRSTS)
        alone = montecarlo.gate_strata_sharded(gadget, STRATA, SAMPLES, SEED, FIRSTS, local_fn=_host)   # no process group
        assert np.array_equal(alone.counts, whole.counts)
        for rank in range(WORLD):                             # every rank holds the whole counts
            got = np.load(tmp_path / ("rank%d.npz" % rank))
            assert tuple(got[name + "_fields"]) == fields
            assert got[name].shape == (len(STRATA), 17, len(fields)) and np.array_equal(got[name], whole.counts), (name, rank)
        assert int(whole.counts[0, 0, 0]) == SAMPLES[0] and 0 < int(whole.counts[2, :, 0].sum()) < SAMPLES[2]
