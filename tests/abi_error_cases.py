"""The argument errors of the 19 solving and creating entry points of the C
ABI: a valid 4 x 4 x 4, r = 2 baseline call of each, and the mutations of one
argument at a time that tests/golden/make_abi_errors.py records from the
parent's library and tests/test_abi_errors.py replays.

A mutation is (name, ((key, value), ...)); a key is an argument's name,
"opts.<field>" or "opts.-<field>" (the field's presence bit cleared).  Two
mutations combine when their keys differ.  Every buffer is sized for the
largest r (17) and dimension (4) any mutation uses, so even a call that a
broken library accepted would stay inside them."""
import ctypes as C

import numpy as np

from tritd import _lib

N, R = 4, 2
NODEV = 6
OBSERVED_NAN = 1  # TRITD_OBSERVED_NAN (include/tritd.h)

SOLVE = "n1 n2 n3 r opts A0 B0 C0"
NCVX = "n1 n2 n3 r rho lambda gamma_A epsilon p theta maxIter tol"
BEST = "A_best B_best C_best valHist valHist1 best_iter stop_reason"
BEST_ALS = "A_best B_best C_best valHist best_iter stop_reason"
SHARD = "ld n1 n2 n3 i0 i1 r opts"
ENTRY_POINTS = {
    "tritd_admm_f64": f"D {SOLVE} A B C O E errHist iters device",
    "tritd_admm_masked_f64": f"D observed {SOLVE} A B C O E errHist iters device",
    "tritd_admm_holdout_f64": f"D observed holdout n1 n2 n3 r opts patience val_norm A0 B0 C0 "
                              f"A B C O E errHist iters {BEST} device",
    "tritd_admm_f32": f"D {SOLVE} A B C O E errHist iters device",
    "tritd_admm_sharded_virtual_f64": f"D {SOLVE} nshards A B C O E errHist iters device",
    "tritd_als_f64": f"X {SOLVE} A B C errHist iters device",
    "tritd_als_masked_f64": f"X observed {SOLVE} A B C errHist iters device",
    "tritd_als_holdout_f64": f"X observed holdout n1 n2 n3 r opts patience A0 B0 C0 A B C errHist "
                             f"iters {BEST_ALS} device",
    "tritd_als_sharded_virtual_f64": f"X {SOLVE} nshards A B C errHist iters device",
    "tritd_ncvx_f64": f"X {NCVX} A0 B0 C0 A B C O errHist iters device",
    "tritd_ncvx_masked_f64": f"X observed {NCVX} A0 B0 C0 A B C O errHist iters device",
    "tritd_ncvx_holdout_f64": f"X observed holdout {NCVX} patience val_norm A0 B0 C0 A B C O "
                              f"errHist iters {BEST} device",
    "tritd_session_create": f"out device D {SHARD} A0 B0 C0 comm flags",
    "tritd_session_create_masked": f"out device D observed {SHARD} A0 B0 C0 comm flags",
    "tritd_session_create_holdout": f"out device D observed holdout {SHARD} patience val_norm "
                                    f"A0 B0 C0 comm flags",
    "tritd_als_session_create": f"out device X {SHARD} A0 B0 C0 comm flags quiet",
    "tritd_als_session_create_masked": f"out device X observed {SHARD} A0 B0 C0 comm flags quiet",
    "tritd_als_session_create_holdout": f"out device X observed holdout {SHARD} patience "
                                        f"A0 B0 C0 comm flags quiet",
    "tritd_als_session_create_ncvx_holdout": f"out device X observed holdout {SHARD} patience "
                                             f"val_norm rho lambda gamma_A epsilon p theta "
                                             f"A0 B0 C0 comm flags quiet",
}

# what a non-pointer argument is in the baseline call
SCALARS = dict(n1=N, n2=N, n3=N, r=R, ld=N, i0=0, i1=N, nshards=2, patience=0, val_norm=2,
               rho=1.1, gamma_A=1e-3, epsilon=1e-3, p=0.5, theta=1.0, maxIter=3, tol=1e-6,
               flags=0, quiet=1, comm=None, **{"lambda": 0.5})
OPTS = dict(mu=1e-3, rho=1.25, lambda_=1.8, lambda2=1e-3, tol=1e-5, maxIter=3, disp=0, model=0)
# the rules of the issue that apply wherever the argument exists
BY_ARGUMENT = dict(
    n1=[("n1=0", 0)], n2=[("n2=0", 0)], n3=[("n3=0", 0)],
    r=[("r=0", 0), ("r=9", 9), ("r=17", 17)],
    patience=[("patience=-1", -1)], val_norm=[("val_norm=3", 3)],
    i0=[("i0>=i1", N)], i1=[("i1>n1", N + 1)], ld=[("ld<shard", N - 1)],
    flags=[("flags=F32", _lib.SESSION_F32), ("flags=PROBE", _lib.SESSION_PROBE),
           ("flags=D_ON_DEVICE", _lib.SESSION_D_ON_DEVICE)],
    nshards=[("nshards=0", 0), ("nshards=17", 17), ("nshards=n1+1", N + 1)],
    observed=[("observed=NAN", OBSERVED_NAN)])


def names(entry):
    return ENTRY_POINTS[entry].split()


def is_pointer(entry, i):
    t = _lib.SIGNATURES[entry][1][i]
    return t is C.c_void_p or hasattr(t, "contents")


def mutations(entry):
    """Every single mutation of the entry point, in a fixed order."""
    out = []
    args = names(entry)
    for i, a in enumerate(args):
        if is_pointer(entry, i) and a != "comm":
            out.append((a + "=NULL", ((a, None),)))
    for a in args:
        if a == "rho":  # (the nonconvex solver's own argument, not opts.rho)
            out.append(("rho=0", (("rho", 0.0),)))
        for name, v in BY_ARGUMENT.get(a, ()):
            out.append((name, ((a, v),)))
    if "opts" in args:
        for f in _lib.OPT_BITS:
            out.append(("opts.%s absent" % f, (("opts.-" + f, None),)))
        out.append(("model=qi", (("opts.model", 1),)))
        out.append(("model=7", (("opts.model", 7),)))
    return out


class Buffers:
    """One set of zero-filled host buffers every call shares (nothing is
    computed: a refused call reads none, an accepted one ends at the missing
    device)."""

    def __init__(self):
        big = N * 17 * 17 * N  # above any factor at r = 17 and the 4 x 4 x 4 tensors
        self.f64 = np.ones(big)
        self.u8 = np.ones(N * N * N, dtype=np.uint8)
        self.u8[::5] = 0
        self.i32 = [C.c_int32(0) for _ in range(3)]
        self.out = C.c_void_p()

    def pointer(self, entry, i, name):
        t = _lib.SIGNATURES[entry][1][i]
        if name in ("observed", "holdout"):
            return C.c_void_p(self.u8.ctypes.data)
        if name == "out":
            return C.byref(self.out)
        if t is C.c_void_p:
            return C.c_void_p(self.f64.ctypes.data)
        return C.byref(self.i32[("iters", "best_iter", "stop_reason").index(name)])


def call(lib, bufs, entry, changes=()):
    """Call the entry point with the baseline arguments and ``changes`` (the
    (key, value) pairs of one or more mutations); -> (status, message)."""
    o = _lib.Opts()
    for f, v in OPTS.items():
        setattr(o, f, v)
    o.present = 0x7F
    values = {}
    for key, v in changes:
        if key.startswith("opts.-"):
            o.present &= ~_lib.OPT_BITS[key[6:]]
        elif key.startswith("opts."):
            setattr(o, key[5:], v)
        else:
            values[key] = v
    args = []
    for i, a in enumerate(names(entry)):
        if a in values:
            v = values[a]
            args.append(C.c_void_p(v) if v is not None and is_pointer(entry, i) else v)
        elif a == "opts":
            args.append(C.byref(o))
        elif a == "device":
            args.append(0 if "out" in names(entry) else -1)
        elif is_pointer(entry, i) and a != "comm":
            args.append(bufs.pointer(entry, i, a))
        else:
            args.append(SCALARS[a])
    bufs.out.value = None
    status = getattr(lib, entry)(*args)
    assert not bufs.out.value or status == 0, "a refused creator left a handle behind"
    return status, lib.tritd_last_error().decode()


def combinable(a, b):
    """two mutations that touch different arguments"""
    return not {k for k, _ in a[1]} & {k for k, _ in b[1]}
