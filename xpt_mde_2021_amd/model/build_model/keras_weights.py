"""Keras weight I/O shared by every DepthNetPretrained backbone: the torch <-> Keras layouts, the weight-file reader, the
variable-naming helpers of a backbone's `keras_variable_map`, and ONE strict export / load over such a map.

A map is {keras variable name: (tensor of the encoder, kind)} with kind in {"conv", "depthwise", "vector"}.  `selections`
({id(tensor): (out_sel, in_sel)}, NASNet-Mobile only) names the tensors that carry structurally-zero entries: the Keras
variables address their logical entries only, the rest is filled with 0 (1 for a moving variance)."""
import torch

from ...utils.util_class import WrongInputException


def _to_keras(kind, t):
    """torch layout -> keras layout: conv OIHW -> HWIO, depthwise [C,1,k,k] -> [k,k,C,1]."""
    if kind == "conv":
        return t.permute(2, 3, 1, 0)
    if kind == "depthwise":
        return t.permute(2, 3, 0, 1)
    return t


def _from_keras(kind, a):
    if kind == "conv":
        return a.permute(3, 2, 0, 1)
    if kind == "depthwise":
        return a.permute(2, 3, 0, 1)
    return a


def bn(out, name, module):
    """The four variables of a BatchNormalization layer."""
    out[f"{name}/gamma"] = (module.weight, "vector")
    out[f"{name}/beta"] = (module.bias, "vector")
    out[f"{name}/moving_mean"] = (module.running_mean, "vector")
    out[f"{name}/moving_variance"] = (module.running_var, "vector")


def conv(out, name, module):
    """The kernel of a Conv2D layer, and its bias when it has one."""
    out[f"{name}/kernel"] = (module.weight, "conv")
    if module.bias is not None:
        out[f"{name}/bias"] = (module.bias, "vector")


def logical_view(t, sel):
    """The logical entries of t (a copy when t carries structural zeros, t itself otherwise)."""
    if sel is None:
        return t
    o, i = sel
    if o is not None:
        t = t.index_select(0, o.to(t.device))
    if i is not None:
        t = t.index_select(1, i.to(t.device))
    return t


def _store_logical(t, sel, value, fill=0.0):
    if sel is None:
        t.copy_(value.to(device=t.device, dtype=t.dtype))
        return
    o, i = sel
    full = torch.full_like(t, fill)
    oo = (o if o is not None else torch.arange(t.shape[0])).to(t.device)
    v = value.to(device=t.device, dtype=t.dtype)
    if i is not None:
        full[oo[:, None], i.to(t.device)[None, :]] = v
    else:
        full[oo] = v
    t.copy_(full)


def read_keras_weight_file(path):
    """{variable name: numpy array} from an .npz keyed by keras variable names (INTEGRATION.md has the one-line export to
    run where Keras is installed) or from Keras' own NASNet-mobile-no-top.h5 when h5py is importable."""
    import numpy as np
    if str(path).endswith(".npz"):
        with np.load(path) as z:
            return {k[:-2] if k.endswith(":0") else k: z[k] for k in z.files}
    if str(path).endswith((".h5", ".hdf5")):
        try:
            import h5py
        except ImportError as e:
            raise WrongInputException("reading a Keras .h5 file needs h5py (not installed): convert it to .npz, "
                                      "INTEGRATION.md") from e
        out = {}
        with h5py.File(path, "r") as f:
            root = f["model_weights"] if "model_weights" in f else f

            def visit(name, obj):
                if isinstance(obj, h5py.Dataset):
                    parts = name.split("/")
                    var = parts[-1][:-2] if parts[-1].endswith(":0") else parts[-1]
                    out[f"{parts[-2]}/{var}"] = obj[()]
            root.visititems(visit)
        return out
    raise WrongInputException(f"unknown weight file type: {path}")


def export_weights(table, selections=None):
    """{keras variable name: float32 array in the keras layout} of the current values of a variable map."""
    sel = selections or {}
    return {name: _to_keras(kind, logical_view(t.detach(), sel.get(id(t)))).contiguous().float().cpu()
            for name, (t, kind) in table.items()}


def load_weights(table, weights, label, selections=None):
    """Fills the tensors of a variable map from Keras variables (a path or a {name: array} dict); `label` names the model in
    the messages.  Strict: a missing, unknown or mis-shaped variable raises; nothing is loaded partially."""
    if not isinstance(weights, dict):
        weights = read_keras_weight_file(weights)
    missing = sorted(set(table) - set(weights))
    unknown = sorted(set(weights) - set(table))
    if missing or unknown:
        raise WrongInputException(f"{label} weights: {len(missing)} variables missing (e.g. {missing[:3]}), "
                                  f"{len(unknown)} not part of the no-top model (e.g. {unknown[:3]})")
    staged = {}
    sel = selections or {}
    for name, (t, kind) in table.items():
        a = torch.as_tensor(weights[name])
        want = tuple(_to_keras(kind, logical_view(t, sel.get(id(t)))).shape)
        if tuple(a.shape) != want:
            raise WrongInputException(f"{name}: file has shape {tuple(a.shape)}, the model expects {want}")
        staged[name] = _from_keras(kind, a)
    with torch.no_grad():
        for name, (t, kind) in table.items():
            _store_logical(t, sel.get(id(t)), staged[name], fill=1.0 if name.endswith("/moving_variance") else 0.0)
    return len(staged)
