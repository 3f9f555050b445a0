"""ctypes binding of libmi355_carla.so, generated from include/mi355_carla.h.

There is NO fallback: if the shared library is missing the import of anything that needs it raises
(the product path must fail loudly without the HIP extension).
"""
import ctypes
import numbers
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
HEADER = os.path.join(ROOT, "include", "mi355_carla.h")
LIB_PATH = os.environ.get("MI355_LIB") or os.path.join(HERE, "libmi355_carla.so")     # MI355_LIB: another build of the same library (tools/asan_host_check.sh)

MI_F32, MI_BF16, MI_BF16X3 = 0, 1, 2              # MI_BF16X3: split storage (two bf16 halves hi | lo per 4-byte element), include/mi355_carla.h
# precision modes of the PPO step (mi_ppo_set_precision): exact fp32, or its GEMM stages on the bf16 matrix pipe as split (hi + lo) fp32 operands
PPO_PRECISIONS = {"fp32": MI_F32, "f32": MI_F32, "bf16x3": MI_BF16X3}


def ppo_precision_name(precision):
    """'fp32' / 'f32' / 'bf16x3' -> the canonical name ('fp32' or 'bf16x3'); anything else raises ValueError."""
    p = str(precision).strip().lower()
    if p not in PPO_PRECISIONS:
        raise ValueError("PPO precision %r: expected one of %s" % (precision, ", ".join(sorted(PPO_PRECISIONS))))
    return "fp32" if p == "f32" else p


def max_grad_norm_value(value, who="max_grad_norm"):
    """The limit of global-norm gradient clipping (mi_ppo_set_max_grad_norm): None (off) or a positive float (inf: measure the norm, never clip) -> None or float;
    bool, str, 0, a negative value or NaN raise ValueError.  No device and no library involved."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not value > 0:      # (numpy's scalar types are registered as numbers.Real)
        raise ValueError("%s: the value is None or a positive float (inf: measure the norm, never clip), got %r" % (who, value))
    return float(value)


def value_clip_value(value, who="value_clip"):
    """The range eps_v of PPO2-style value-function clipping (mi_ppo_train_step_vclip): None (off) or a positive float (inf: the clipped entry, never a clipped
    sample) -> None or float; bool, str, 0, a negative value or NaN raise ValueError.  No device and no library involved."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not value > 0:
        raise ValueError("%s: the value is None or a positive float (inf: the value is never clipped), got %r" % (who, value))
    return float(value)


def dual_clip_value(value, who="dual_clip"):
    """The constant c of dual-clip PPO (mi_ppo_set_dual_clip): None (off) or a float > 1 (inf: the setting is on and no sample is ever dual-clipped) -> None or
    float; bool, str, NaN or a value <= 1 raise ValueError.  No device and no library involved."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not value > 1:
        raise ValueError("%s: the value is None or a float > 1 (inf: no sample is ever dual-clipped), got %r" % (who, value))
    return float(value)


def loss_coef_values(clip_eps, value_scale, entropy_scale, who="loss_coefs"):
    """The three loss coefficients of the PPO step (mi_ppo_set_loss_coefs): clip_eps finite and > 0, value_scale and entropy_scale finite and >= 0 -> three floats;
    bool, str, NaN, inf or a value outside its range raise ValueError.  No device and no library involved."""
    out = []
    for name, value, positive in (("clip_eps", clip_eps, True), ("value_scale", value_scale, False), ("entropy_scale", entropy_scale, False)):
        ok = not isinstance(value, bool) and isinstance(value, numbers.Real) and value < float("inf") and (value > 0 if positive else value >= 0)
        if not ok:
            raise ValueError("%s: %s is a finite float %s 0, got %r" % (who, name, ">" if positive else ">=", value))
        out.append(float(value))
    return tuple(out)


def kl_penalty_value(value, who="kl_penalty"):
    """The coefficient beta of the KL penalty (mi_ppo_train_step_kl): None (off) or a finite float >= 0 (0: the penalised step, nothing added: it measures the KL)
    -> None or float; bool, str, a negative value, inf or NaN raise ValueError.  No device and no library involved."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not (value >= 0 and value < float("inf")):
        raise ValueError("%s: the value is None or a finite float >= 0 (0: measure the KL, add nothing), got %r" % (who, value))
    return float(value)


def kl_target_value(value, who="kl_target"):
    """The target of the adaptive KL penalty: None (beta stays fixed) or a finite float > 0 -> None or float; anything else raises ValueError."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not (value > 0 and value < float("inf")):
        raise ValueError("%s: the value is None (a fixed coefficient) or a finite float > 0, got %r" % (who, value))
    return float(value)


CLONE_KINDS = {"nll": 0, "mse": 1}                # `kind` of mi_ppo_clone_step


def clone_kind(loss, who="clone_step"):
    """The loss of a behaviour-cloning step (mi_ppo_clone_step): "nll" or "mse" (or the C entry's 0 / 1) -> 0 / 1; anything else raises ValueError.  No device and
    no library involved."""
    if isinstance(loss, str) and loss in CLONE_KINDS:
        return CLONE_KINDS[loss]
    if not isinstance(loss, (bool, str)) and isinstance(loss, numbers.Integral) and int(loss) in (0, 1):
        return int(loss)
    raise ValueError('%s: the loss is "nll" (the Gaussian negative log-likelihood) or "mse" (the squared error of the action mean), got %r' % (who, loss))


_CTYPES = {
    "void*": ctypes.c_void_p, "const void*": ctypes.c_void_p,
    "float*": ctypes.c_void_p, "const float*": ctypes.c_void_p,
    "double*": ctypes.c_void_p, "const double*": ctypes.c_void_p,
    "int*": ctypes.c_void_p, "const int*": ctypes.c_void_p,
    "char*": ctypes.c_char_p, "const char*": ctypes.c_char_p, "const unsigned char*": ctypes.c_void_p,
    "int": ctypes.c_int, "unsigned int": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong,
    "long long*": ctypes.c_void_p, "const long long*": ctypes.c_void_p, "void": None,
    "unsigned long long": ctypes.c_ulonglong, "unsigned long long*": ctypes.c_void_p,
    "void**": ctypes.c_void_p, "unsigned char*": ctypes.c_void_p, "void* const*": ctypes.c_void_p, "void*const*": ctypes.c_void_p,
    "const MiVaeDesc*": ctypes.c_void_p, "const MiPpoDesc*": ctypes.c_void_p, "const MiMlpVaeDesc*": ctypes.c_void_p,
}


class MiVaeDesc(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int), ("max_batch", ctypes.c_int), ("ih", ctypes.c_int), ("iw", ctypes.c_int),
                ("cin", ctypes.c_int), ("ct", ctypes.c_int), ("z_dim", ctypes.c_int), ("loss_kind", ctypes.c_int),
                ("beta", ctypes.c_float), ("kl_tolerance", ctypes.c_float), ("inference_only", ctypes.c_int)]


MI_MLP_MAX_HIDDEN = 4


class MiMlpVaeDesc(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int), ("max_batch", ctypes.c_int), ("source_size", ctypes.c_int), ("target_size", ctypes.c_int), ("z_dim", ctypes.c_int),
                ("n_enc", ctypes.c_int), ("n_dec", ctypes.c_int), ("enc", ctypes.c_int * MI_MLP_MAX_HIDDEN), ("dec", ctypes.c_int * MI_MLP_MAX_HIDDEN),
                ("loss_kind", ctypes.c_int), ("with_optimizer", ctypes.c_int), ("beta", ctypes.c_float), ("kl_tolerance", ctypes.c_float)]


class MiPpoDesc(ctypes.Structure):
    _fields_ = [("max_batch", ctypes.c_int), ("input_dim", ctypes.c_int), ("num_actions", ctypes.c_int),
                ("h1", ctypes.c_int), ("h2", ctypes.c_int), ("clip_eps", ctypes.c_float),
                ("value_scale", ctypes.c_float), ("entropy_scale", ctypes.c_float)]


class MiError(RuntimeError):
    pass


def parse_header(path=HEADER):
    """-> {name: (restype_str, [(argtype_str, argname), ...])} for every prototype in the header."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for m in re.finditer(r"^\s*((?:const\s+)?\w[\w\s]*?\**)\s*(mi_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        ret = re.sub(r"\s*\*", "*", ret)
        arglist = []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                mm = re.match(r"^(.*?)(\w+)$", a)
                typ = re.sub(r"\s*\*\s*", "*", mm.group(1).strip())
                arglist.append((typ, mm.group(2)))
        protos[name] = (ret, arglist)
    return protos


class _Lib:
    def __init__(self):
        if not os.path.exists(LIB_PATH):
            raise MiError("libmi355_carla.so not found at %s — run `python __graft_entry__.py` (build()) first; "
                          "there is no CPU fallback" % LIB_PATH)
        # PyTorch first: it bundles its own libamdhip64.so.7 / libhsa-runtime64 and every device buffer this library is handed comes from it.  Loaded
        # the other way round, the loader binds BOTH to the system ROCm's runtime (same SONAME) and PyTorch's build then finds no device.
        import torch  # noqa: F401
        self.cdll = ctypes.CDLL(LIB_PATH)
        self.protos = parse_header()
        self.cdll.mi_last_error.restype = ctypes.c_char_p
        self._check_structs = True
        for name, (ret, args) in self.protos.items():
            fn = getattr(self.cdll, name)          # AttributeError if the header declares a symbol the .so lacks
            fn.restype = _CTYPES[ret]
            fn.argtypes = [_CTYPES[t] for t, _ in args]
            if ret == "int" and not name.endswith(("_version", "_chunks", "_blocks", "_floats", "_bytes", "_count", "_size", "_tuning", "_ok", "_offset", "_rsag", "_recorded", "_bias_rows")):
                setattr(self, name, self._checked(name, fn))
            else:
                setattr(self, name, fn)

    def check_struct_sizes(self):
        assert self.mi_vae_desc_size() == ctypes.sizeof(MiVaeDesc), "MiVaeDesc layout mismatch between header and binding"
        assert self.mi_ppo_desc_size() == ctypes.sizeof(MiPpoDesc), "MiPpoDesc layout mismatch between header and binding"
        assert self.mi_mlpvae_desc_size() == ctypes.sizeof(MiMlpVaeDesc), "MiMlpVaeDesc layout mismatch between header and binding"

    def _checked(self, name, fn):
        def call(*a):
            rc = fn(*a)
            if rc != 0:
                raise MiError("%s failed (%d): %s" % (name, rc, self.cdll.mi_last_error().decode()))
            return rc
        call.__name__ = name
        return call


_lib = None


def get():
    global _lib
    if _lib is None:
        _lib = _Lib()
        _lib.check_struct_sizes()
    return _lib


def ptr(t):
    """Device (or host) pointer of a torch tensor / None -> int for ctypes."""
    return None if t is None else t.data_ptr()
