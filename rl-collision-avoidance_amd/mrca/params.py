"""What the Python mirrors of the library's params structs (include/mrca_env.h: mrca_orca_params ... mrca_planner_params) share.
A mirror is a dataclass on ``ParamsMirror`` that declares the struct's fields, all ``None``, and names three things: its ctypes
struct (``_STRUCT``), the export that fills in the library's defaults (``_DEFAULTS`` -- they are stated once, in C) and the
command-line flag its assignments come from (``_FLAG``)."""
import ctypes as C

from . import _lib

_defaults = {}      # mirror class -> {field: the library's default}


class ParamsMirror:
    _STRUCT = _DEFAULTS = _FLAG = None
    _SHORT = {}     # other names the command line knows a field by

    @classmethod
    def _types(cls):
        return {k: (int if t is C.c_int32 else float) for k, t in cls._STRUCT._fields_}

    @classmethod
    def library_defaults(cls):
        if cls not in _defaults:
            st = cls._STRUCT()
            _lib.check(getattr(_lib.load(), cls._DEFAULTS)(C.byref(st)), cls._DEFAULTS)
            _defaults[cls] = {k: getattr(st, k) for k in cls._types()}
        return _defaults[cls]

    def __post_init__(self):
        """A field left ``None`` takes the library's default; an integer field is an ``int``."""
        for k, v in self.library_defaults().items():
            if getattr(self, k) is None:
                setattr(self, k, v)
            if self._types()[k] is int:
                setattr(self, k, int(getattr(self, k)))

    def as_dict(self):
        return {k: t(getattr(self, k)) for k, t in self._types().items()}

    def struct(self):
        return self._STRUCT(**self.as_dict())

    @classmethod
    def from_assignments(cls, items, start=None):
        """``["name=value", ...]`` (what ``_FLAG`` collects) on top of the fields of ``start`` -> an instance."""
        types = cls._types()
        kw = dict(start or {})
        for it in items or ():
            k, eq, v = it.partition("=")
            k = cls._SHORT.get(k, k)
            if k not in types or not eq:
                raise ValueError(f"{cls._FLAG} {it!r}: expected name=value with name in {sorted(cls._SHORT) + list(types)}")
            kw[k] = types[k](v)
        return cls(**kw)
