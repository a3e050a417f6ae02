"""Guard-band cases of the experimental header include/experimental/plnerf_hip_dpstep.h, described with the machinery of
tests/containment.py (imported, not edited: that table is the registered ABI's), as tests/camcode_cases.py does for its
header.  tests/test_gpu_one_call_dp.py runs each through containment.run_case; tests/test_dpstep_abi.py builds them on the
CPU, holds every call to its prototype and requires a case for every entry of the header that takes a stream.

A case is the registered one-call step's own case (containment.train_step_case / depth_step_case: two steps of 67 then 41
rays on a workspace of exactly the size query's bytes, the second depth step also stepping the scales and shifts) with every
call cut in two: `*_grads` on the call's own arguments, then `*_apply` on its three structs with a grad_scale of 0.5.  In
`apply` the gradient blocks are inputs: it must leave them what `grads` wrote."""
import containment as C
from containment import IN, INOUT, Call, Struct

NO_DEVICE_WRITES = set()      # every entry of the header takes a stream
GRAD_SCALE = 0.5


def _split(calls, apply_entry):
    out = []
    for call in calls:
        cfg, io, args = call.args[:3]
        # what apply touches of io: parameters and moments (inout), the gradient blocks (in); the depth step's scales, shifts
        # and their moments keep the roles the whole step gave them
        refs = []
        for r in io.refs:
            name = r.buf.name
            if name.endswith("grad_flat") or name == "ss_grad":
                refs.append(IN(r.buf, r.offset))
            elif r.role == "inout":      # (parameters, moments; on a step of theirs the scales, shifts and their moments)
                refs.append(INOUT(r.buf, r.offset))
        out.append(Call(call.entry + "_grads", *call.args))
        out.append(Call(apply_entry, cfg, Struct(refs, io.build), Struct(list(args.refs), args.build), GRAD_SCALE))
    return out


def train_case(L, mode):
    return _split(C.train_step_case(L, mode), "plnerf_train_step_apply")


def depth_case(L, constant):
    return _split(C.depth_step_case(L, constant), "plnerf_depth_train_step_apply")


def all_cases():
    """(case id, builder taking the binding) of every guard-band case of the header."""
    return [("dp_train_step", lambda L: train_case(L, C.MODE_LINEAR)),
            ("dp_train_step_const", lambda L: train_case(L, C.MODE_CONSTANT)),
            ("dp_depth_train_step", lambda L: depth_case(L, False)),
            ("dp_depth_train_step_const", lambda L: depth_case(L, True))]
