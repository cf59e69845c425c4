from .BMGP import BMGP, MultitaskBMGP                    # voltron/models/__init__.py:1-6 (hot-path subset)
from .VoltronGP import VoltronGP
from .single_task_variational_gp import SingleTaskVariationalGP
from .VoltMagpie import VoltMagpie
from .multi_task_variational_gp import MultitaskVariationalGP


def __getattr__(name):                                   # MaternGP / SMGP (voltron/models/__init__.py:5): out of scope, but
    from .._out_of_scope import resolve                  # the reference's drivers import them unconditionally
    if name in ("MaternGP", "SMGP"):
        return resolve(name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
