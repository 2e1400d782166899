"""ctypes binding of librrl_hip.so.  The C ABI is declared once, in include/rrl.h: the argument lists, structures and
constants below are what _abi.py reads there, so an entry declared in the header and defined in csrc/ needs no line here.

There is NO fallback: if the library is missing, or no MI355X is visible, every op raises.
"""
import ctypes
import os

import torch  # noqa: F401  -- FIRST: librrl_hip.so must bind to the libamdhip64 PyTorch loaded,
#                              or its streams / device pointers belong to another HIP runtime

from ._abi import CONSTANTS, PROTOS, STRUCTS
from .build import LIB

_SIGS = {name: args for name, (res, args) in PROTOS.items() if res is ctypes.c_int}  # name -> argtypes of the entries that return int
EXPORTS = sorted(PROTOS)

# The header's constants that Python uses, under their names without RRL_ (one the header no longer defines: KeyError here).
#   F_*: rrl_opts.flags; GROUP_*: rrl_ball_group's features; MCTL_ERR / CHAIN_TIMEOUT: the control words of a sample's MCTL /
#   CHAIN row that Python reads; FIT_*: rrl_kabsch_fwd's fit [B][32] doubles and info[b][1]; PLANE_*: rrl_plane_normal_eq's
#   neq [B][32] doubles; PLANE_STEPPED.., NEWTON_*, ICP_DONE: state[b][3] of the pose loops' step entries
for _name in ("F_TARGET_KEPT F_CHAIN F_CHAINED GROUP_XYZ GROUP_DXYZ GROUP_PPF GROUP_MAX_SAMPLE MCTL_ERR CHAIN_TIMEOUT "
              "FIT_W FIT_ABAR FIT_BBAR FIT_U FIT_S FIT_V FIT_DELTA FIT_RES FIT_KEYMEAN FIT_DOUBLES FIT_OK FIT_FEW FIT_DEGENERATE "
              "ICP_DONE PLANE_H PLANE_G PLANE_W PLANE_RES PLANE_KEYMEAN PLANE_USED PLANE_SKIPPED PLANE_DOUBLES "
              "PLANE_STEPPED PLANE_FEW PLANE_FAILED PLANE_DONE NEWTON_STEPPED NEWTON_GATED NEWTON_FAILED NEWTON_DONE").split():
    globals()[_name] = CONSTANTS["RRL_" + _name]


class ChamferRider(ctypes.Structure):
    """include/rrl.h rrl_chamfer_rider: the evaluation's Chamfer walk, carried by its culled scan's launch."""
    _fields_ = STRUCTS["rrl_chamfer_rider"]


class Opts(ctypes.Structure):
    """include/rrl.h rrl_opts: the per-call options of the *_ex entry points (-1 / NULL = the library default)."""
    _fields_ = STRUCTS["rrl_opts"]

    def __init__(self, flags=0, reduce_mode=-1, deterministic=-1, sort_parts=-1, scan_variant=-1, order1=None,
                 order2=None, scan_counters=None, scan_counter_rows=0, chamfer=None, payload=None, problems=0,
                 chain_left=None, count1=None, count2=None, nlines=None):
        super().__init__(struct_bytes=ctypes.sizeof(Opts), flags=int(flags), reduce_mode=int(reduce_mode),
                         deterministic=int(deterministic), sort_parts=int(sort_parts), scan_variant=int(scan_variant),
                         order1=order1, order2=order2, scan_counters=scan_counters, scan_counter_rows=int(scan_counter_rows),
                         chamfer=chamfer, payload=payload, problems=int(problems), chain_left=chain_left, count1=count1,
                         count2=count2, nlines=nlines)


# every other structure of the header: rrl_demo_epoch_args -> DemoEpochArgs, rrl_kabsch_args -> KabschArgs, ...
for _name, _fields in STRUCTS.items():
    _camel = "".join(word.capitalize() for word in _name.split("_")[1:])
    if _camel not in globals():
        globals()[_camel] = type(_camel, (ctypes.Structure,), {"_fields_": _fields, "__doc__": f"include/rrl.h {_name}."})

_lib = None


class RRLError(RuntimeError):
    pass


def load():
    """Load librrl_hip.so; raises RRLError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB):
        raise RRLError(
            f"{LIB} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). "
            "This package has no CPU or PyTorch fallback.")
    lib = ctypes.CDLL(LIB)
    for name, (res, args) in PROTOS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def check(rc, what):
    if rc == 0:
        return
    if rc < 0:
        raise RRLError(f"{what}: argument error {rc} (see RRL_E_* in include/rrl.h)")
    raise RRLError(f"{what}: HIP error {rc}")
