"""Tests-only helpers of the IPPO device path: the host build of resco_amd/csrc/resco_ppo.h (tests/ppo_host) and the truth its
results are measured against -- gae() and the standardisation of BatchedPPOLearner.make_dataset (resco_amd/agents/ippo.py:133-145,
175-177), evaluated by those very functions in float64 (truth) and in float32 (whose distance from the truth is the yardstick)."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

from resco_amd.agents.ippo import gae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_ppo_host(out_dir):
    out = os.path.join(str(out_dir), 'ppo_host.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fno-fast-math', '-shared',
                           '-I' + os.path.join(ROOT, 'resco_amd', 'csrc'), os.path.join(ROOT, 'tests', 'ppo_host', 'ppo_host.cpp'), '-o', out])
    L = C.CDLL(out)
    vp, i32 = C.c_void_p, C.c_int32
    L.ppo_gae.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_float, C.c_float, vp, vp, vp]
    return L


def host_gae(L, rew, val, last, done, gamma=0.99, lambd=0.95):
    """numpy float32 [T, N, S] x 2, [N, S], bool [T] -> (adv standardised, ret) of the host build"""
    T, N, S = rew.shape
    rew, val, last = (np.ascontiguousarray(a, np.float32) for a in (rew, val, last))
    d8 = np.ascontiguousarray(done, np.uint8)
    adv, ret, scratch = np.empty_like(rew), np.empty_like(rew), np.empty((N, S), np.float32)
    rc = L.ppo_gae(rew.ctypes.data, val.ctypes.data, last.ctypes.data, d8.ctypes.data, T, N, S, gamma, lambd, adv.ctypes.data,
                   ret.ctypes.data, scratch.ctypes.data)
    assert rc == 0
    return adv, ret


def torch_gae(rew, val, last, done, dtype, gamma=0.99, lambd=0.95):
    """gae() + make_dataset's standardisation in `dtype` -> numpy (adv standardised, ret), both [T, N, S]"""
    r, v, l = (torch.as_tensor(a).to(dtype) for a in (rew, val, last))
    adv, ret = gae(r, v, l, torch.as_tensor(done), gamma, lambd)
    T, N, S = adv.shape
    a = adv.reshape(T * N, S)
    a = (a - a.mean(0, keepdim=True)) / (a.std(0, unbiased=False, keepdim=True) + 1e-8)
    return a.reshape(T, N, S).numpy(), ret.numpy()


def gae_case(T=32, N=48, S=5, seed=0):
    """random fp32 inputs, done at one interior step and at the last one"""
    rng = np.random.default_rng(seed)
    rew = rng.standard_normal((T, N, S)).astype(np.float32)
    val = rng.standard_normal((T, N, S)).astype(np.float32)
    last = rng.standard_normal((N, S)).astype(np.float32)
    done = np.zeros(T, bool)
    done[T // 3] = True
    done[T - 1] = True
    return rew, val, last, done


def gae_errors(adv, ret, rew, val, last, done):
    """(error of adv, of ret, e_ref of adv, e_ref of ret): max |x - truth| for the candidate and for torch's own fp32 evaluation"""
    ta, tr = torch_gae(rew, val, last, done, torch.float64)
    fa, fr = torch_gae(rew, val, last, done, torch.float32)
    return (np.abs(adv - ta).max(), np.abs(ret - tr).max(), np.abs(fa - ta).max(), np.abs(fr - tr).max())
