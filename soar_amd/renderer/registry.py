"""Minimal stand-in for the threestudio plugin registry (the `submodules/threestudio` directory of the reference is an
empty submodule).  Used ONLY when the real package cannot be imported; the surface is what the SOAR extension touches:
``threestudio.register(name)``, ``threestudio.find(name)``, ``threestudio.info(msg)``, and a ``BaseObject`` and a ``BaseModule``
(the same as an ``nn.Module``: the background) whose constructors parse ``cfg`` into the nested ``Config`` dataclass and call
``configure()``."""
from __future__ import annotations

import dataclasses
import logging
from typing import Any, Dict, Optional

from torch import nn

try:                                    # pragma: no cover - not installed in this image
    import threestudio as _ts
    register, find, info = _ts.register, _ts.find, _ts.info
    from threestudio.utils.base import BaseModule, BaseObject
    HAVE_THREESTUDIO = True
except Exception:
    HAVE_THREESTUDIO = False
    __modules__: Dict[str, Any] = {}
    _log = logging.getLogger("soar_amd")

    def register(name: str):
        def deco(cls):
            __modules__[name] = cls
            return cls
        return deco

    def find(name: str):
        return __modules__[name]

    def info(msg: str):
        _log.info(msg)

    def _parse(obj, cfg: Optional[dict]):
        fields = {f.name for f in dataclasses.fields(obj.Config)}
        cfg = dict(cfg or {})
        unknown = set(cfg) - fields
        if unknown:
            raise ValueError(f"unknown config keys for {type(obj).__name__}: {sorted(unknown)}")
        return obj.Config(**cfg)

    class BaseObject:
        @dataclasses.dataclass
        class Config:
            pass

        cfg: "BaseObject.Config"

        def __init__(self, cfg: Optional[dict] = None, *args, **kwargs):
            self.cfg = _parse(self, cfg)
            self.device = kwargs.pop("device", None)
            self.configure(*args, **kwargs)

        def configure(self, *args, **kwargs) -> None:
            pass

    class BaseModule(nn.Module):
        @dataclasses.dataclass
        class Config:
            pass

        cfg: "BaseModule.Config"

        def __init__(self, cfg: Optional[dict] = None, *args, **kwargs):
            super().__init__()
            self.cfg = _parse(self, cfg)
            self.configure(*args, **kwargs)

        def configure(self, *args, **kwargs) -> None:
            pass
