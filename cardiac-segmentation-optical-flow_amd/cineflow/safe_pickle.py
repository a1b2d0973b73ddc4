"""Restricted un-pickling of files other pipelines wrote (nnU-Net property `.pkl` files, `plans.pkl`, `<chk>.model.pkl`).

`PlainUnpickler.find_class` resolves only the globals listed in `_ALLOWED`: plain containers and numpy's array / dtype / scalar
reconstructors.  A pickle that names any other global raises `pickle.UnpicklingError` instead of importing or calling it.
Subclasses widen the list with further plain-data globals (cineflow.reference_models)."""
import pickle


class PlainUnpickler(pickle.Unpickler):
    """pickle.Unpickler that can only rebuild plain containers and numpy values (what nnU-Net property dicts hold).  `pkl_path` is a free
    CLI argument and its natural input is a tree another pipeline wrote, so no global outside this list is ever resolved."""

    _ALLOWED = {
        ("collections", "OrderedDict"),
        ("numpy", "ndarray"), ("numpy", "dtype"),
        ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
        ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
        ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer"),
    }
    _WHAT = "a properties .pkl"

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError("refusing to load global %s.%s from %s (plain containers and numpy values only)" % (module, name, self._WHAT))


def load_plain_pickle(path, unpickler=PlainUnpickler):
    with open(path, "rb") as f:
        return unpickler(f).load()
