"""What the tests of the torch-free C++ hosts (tests/c_abi_*_gpu.cpp) share: the one g++ command line that builds a host,
the one way to run it, the numpy restatement of tests/c_abi_host.h's hash and weight fill, the tables file, the checksums
and the parsers of what the hosts print.  tests/test_c_hosts_host.py holds the restatement to the header's bits."""
import os
import subprocess

import numpy as np
import torch

import abi_support as abi

HOSTS = ("c_abi_gpu", "c_abi_step_gpu", "c_abi_const_step_gpu", "c_abi_depth_step_gpu", "c_abi_view_gpu", "c_abi_depth_view_gpu")


def build(name, out_dir, source=None):
    """Compile tests/<name>.cpp (or `source`, a .cpp path) against include/, tests/c_abi_host.h, the built library and the HIP
    runtime; returns the executable's path.  (ISO mode and no fast-math: the hosts' float arithmetic equals numpy's.)"""
    exe = os.path.join(str(out_dir), name)
    libdir = os.path.dirname(abi.built_lib().LIB_PATH)
    tests = os.path.join(abi.ROOT, "tests")
    done = subprocess.run(["g++", "-std=c++17", "-O1", "-I", abi.INCLUDE, "-I", "/opt/rocm/include", "-I", tests,
                           str(source or os.path.join(tests, name + ".cpp")), "-o", exe, "-L", libdir, "-lplnerf_hip",
                           "-L", "/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    return exe


def run(exe, *argv):
    """One run of a host under a limit of its own, never repeated; the completed process, for the caller to assert on."""
    return subprocess.run(["timeout", "-k", "10", "300", exe] + [str(a) for a in argv], capture_output=True, text=True)


def hashed(k, n):
    """tests/c_abi_host.h's hashed(k, i) for i in [0, n)."""
    i = np.arange(n, dtype=np.uint32)
    with np.errstate(over="ignore"):
        x = i * np.uint32(2654435761) + np.uint32((k * 0x9e3779b9) & 0xffffffff) + np.uint32(12345)
        x = x * np.uint32(1664525) + np.uint32(1013904223)
        x ^= x >> np.uint32(15)
        x = x * np.uint32(1664525) + np.uint32(1013904223)
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def step_scene(img_h, img_w):
    """The one view tests/c_abi_step_gpu.cpp and tests/c_abi_const_step_gpu.cpp train on, on the host: (K, c2w [3, 4], the
    image [img_h, img_w, 3] of hashed(999, .))."""
    K = [[60.0, 0, 0.5 * img_w], [0, 60.0, 0.5 * img_h], [0, 0, 1]]
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 4.0]])
    return K, c2w, torch.from_numpy(hashed(999, img_h * img_w * 3)).reshape(img_h, img_w, 3)


def hashed_state_dict(which, shapes):
    """tests/c_abi_host.h's hashed_net_values(which, ...) as a state_dict; `shapes` is the ordered (name, shape) list."""
    by_name, sd = dict(shapes), {}
    for k, (name, shape) in enumerate(shapes):
        fan_in = shape[1] if len(shape) == 2 else by_name[name.replace("bias", "weight")][1]
        bound = np.float32(1.0) / np.sqrt(np.float32(fan_in))
        vals = (np.float32(2.0) * hashed(100 * which + k, int(np.prod(shape))) - np.float32(1.0)) * bound
        sd[name] = torch.from_numpy(vals.astype(np.float32)).reshape(*shape)
    return sd


def write_tables(path, Ns, Ni):
    """t_vals [Ns] then u_vals [Ni], torch.linspace(0, 1, n) to the bit, as the hosts read them."""
    from plnerf_amd import functional as Fn
    with open(str(path), "wb") as f:
        f.write(torch.cat([Fn.cpu_linspace(Ns, "cpu"), Fn.cpu_linspace(Ni, "cpu")]).numpy().tobytes())
    return str(path)


def fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def bits(t):
    """The bit pattern of a one-element fp32 tensor."""
    return int(t.detach().cpu().view(torch.int32).item()) & 0xffffffff


def checksum(t):
    """The sum of an fp32 tensor's bit patterns (the hosts' `params` and `ss` values)."""
    return int(t.detach().reshape(-1).cpu().view(torch.int32).numpy().view(np.uint32).astype(np.uint64).sum())


def parse_steps(stdout):
    """[(total's bits, second value's bits)] of the `step <k> loss <hex> <label> <hex>` lines."""
    return [(int(l.split()[3], 16), int(l.split()[5], 16)) for l in stdout.split("\n") if l.startswith("step ")]


def parse_sums(stdout, tag):
    """The integers of the line `<tag> <int> <int> ...`; a ValueError where there is none."""
    for l in stdout.split("\n"):
        if l.startswith(tag + " "):
            return [int(x) for x in l.split()[1:]]
    raise ValueError(f"no '{tag}' line in the host's output")


def parse_planes(stdout):
    """{plane: hash} of the `<plane> <hex>` lines."""
    return {line.split()[0]: int(line.split()[1], 16) for line in stdout.split("\n") if line.strip()}
