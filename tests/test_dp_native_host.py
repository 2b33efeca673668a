"""CPU: the host side of the data-parallel step driven by the library (include/v2xgnn.h, "data parallelism driven by the
library"): the ctypes v2x_comm against the header, the form constants, the trainer's switches.  Nothing here calls RCCL."""
import ctypes as C
import os
import re

import numpy as np

from v2xgnn import lib as vlib
from v2xgnn.dp import DataParallelTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    hdr = open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read()
    return re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)


def test_comm_struct_matches_the_header_field_for_field():
    body = re.search(r'typedef struct v2x_comm \{([^}]*)\} v2x_comm;', _header(), re.S).group(1)
    names = []
    for decl in (d.strip() for d in body.split(';') if d.strip()):
        fn = re.match(r'int\s*\(\*\s*(\w+)\)\s*\(float\*\s*\w+,\s*int64_t\s*\w+,\s*void\*\s*\w+,\s*void\*\s*\w+\)$', decl)
        if fn:
            names.append(fn.group(1))
        else:
            names += re.findall(r'\b([A-Za-z_0-9]+)\s*(?:,|$)', decl.replace('*', ' '))
    assert names == [f[0] for f in vlib.Comm._fields_], names
    # int32 world, rank; one pointer; three function pointers
    assert C.sizeof(vlib.Comm) == 2 * 4 + 8 + 3 * 8
    assert [C.sizeof(t) for _, t in vlib.Comm._fields_[:2]] == [4, 4]
    assert vlib.COLLECTIVE._restype_ is C.c_int and vlib.COLLECTIVE._argtypes_ == (C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)


def test_form_and_error_constants_match_the_header():
    hdr = _header()
    defs = dict((k, int(v)) for k, v in re.findall(r'#define\s+(V2X_DP_\w+|V2X_ECOMM)\s+(-?\d+)', hdr))
    assert defs == {"V2X_DP_ALLREDUCE": vlib.V2X_DP_ALLREDUCE, "V2X_DP_BUCKETS": vlib.V2X_DP_BUCKETS,
                    "V2X_DP_SHARDED": vlib.V2X_DP_SHARDED, "V2X_ECOMM": vlib.V2X_ECOMM}
    assert vlib.V2X_ECOMM == -5 and issubclass(vlib.V2XCommError, vlib.V2XError)
    # the bindings of the new entry points: argument counts as declared
    sym = {n: a for n, _, a in vlib.SYMBOLS}
    assert len(sym["v2x_train_step_dp"]) == 10 and len(sym["v2x_dqn_step_dp"]) == 13
    assert sym["v2x_comm_rccl_create"][-1] == C.POINTER(vlib.Comm)


def test_ecomm_raises_the_comm_error():
    class FakeLib(object):
        def v2x_last_error(self, h):
            return b"all_reduce_sum of bucket 1 (64 floats) returned -1"
    try:
        vlib.check(FakeLib(), vlib.V2X_ECOMM)
    except vlib.V2XCommError as exc:
        assert "bucket 1" in str(exc) and "-5" in str(exc)
    else:
        raise AssertionError("no exception")


class _Backend(object):
    """records what the trainer asks of the engine"""
    device = 0

    def __init__(self):
        self.calls = []

    def train_step_dp(self, batch, y, comm, form, n_global, want_loss):
        self.calls.append((comm, form, n_global, want_loss))
        return np.zeros(2, np.float32)


def test_trainer_is_not_native_by_default_and_picks_the_form_of_its_switches():
    assert DataParallelTrainer(_Backend()).native is False
    comm = object()
    for kw, form in (({}, vlib.V2X_DP_ALLREDUCE), (dict(overlap=True), vlib.V2X_DP_BUCKETS),
                     (dict(shard_optimizer=True), vlib.V2X_DP_SHARDED), (dict(overlap=True, shard_optimizer=True), vlib.V2X_DP_SHARDED)):
        be = _Backend()
        tr = DataParallelTrainer(be, native=True, comm=comm, **kw)
        assert tr.form == form
        tr.train_step("batch", "y", n_graphs_global=512, want_loss=False)
        assert be.calls == [(comm, form, 512, False)]


def test_data_parallel_true_still_builds_the_python_trainer():
    from v2xgnn import GnnSpec, GnnQModel
    from oracle import compact as oc
    from oracle_engine import OracleEngine
    from util import ospec
    spec = GnnSpec(n_nodes=4, feat_dim=16)
    P = oc.init_params(ospec(spec), np.random.default_rng(0))
    for dp, native in ((True, False), ("native", True)):
        model = GnnQModel(spec, engine=OracleEngine(spec, P), data_parallel=dp)
        assert isinstance(model.trainer, DataParallelTrainer) and model.trainer.native is native
    assert GnnQModel(spec, engine=OracleEngine(spec, P)).trainer is None


def test_library_has_no_link_time_rccl_dependency():
    """RCCL is resolved at run time (dlopen), so libv2xgnn.so loads where RCCL is absent: no DT_NEEDED entry names it."""
    data = open(vlib.library_path(), 'rb').read()
    import struct
    assert data[:4] == b'\x7fELF' and data[4] == 2                  # 64-bit little-endian
    shoff, = struct.unpack_from('<Q', data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from('<HHH', data, 0x3A)
    secs = [struct.unpack_from('<IIQQQQIIQQ', data, shoff + i * shentsize) for i in range(shnum)]
    dyn = [s for s in secs if s[1] == 6]                             # SHT_DYNAMIC
    assert len(dyn) == 1
    strtab = secs[dyn[0][6]]                                         # sh_link: its string table
    needed = []
    for off in range(dyn[0][4], dyn[0][4] + dyn[0][5], 16):
        tag, val = struct.unpack_from('<qQ', data, off)
        if tag == 0:
            break
        if tag == 1:                                                 # DT_NEEDED
            s0 = strtab[4] + val
            needed.append(data[s0:data.index(b'\0', s0)].decode())
    assert needed and not any('rccl' in n or 'nccl' in n for n in needed), needed
