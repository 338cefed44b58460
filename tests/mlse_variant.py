"""Copies of an equaliser's float32 model with one expression changed, for the tests that show their grading can fail
(tests/test_mlse_ref.py, test_mlse_div_model.py, test_mlse_irc_model.py)."""
import inspect
import types

import mlse_core


def variant(model, change=None):
    """A copy of the module `model` and of tests/mlse_core.py, which the copy then calls through its name `core`, with the
    expression change[0] -- it has to stand exactly once in the two texts together -- replaced by change[1] (None: unchanged
    copies); compiled here and never stored."""
    src = [inspect.getsource(m) for m in (mlse_core, model)]
    if change is not None:
        old, new = change
        assert sum(s.count(old) for s in src) == 1, "%s and mlse_core no longer contain %r exactly once" % (model.__name__, old)
        src = [s.replace(old, new) for s in src]
    core, mod = types.ModuleType("mlse_core_variant"), types.ModuleType(model.__name__ + "_variant")
    exec(compile(src[0], "<variant of mlse_core: %r>" % (change,), "exec"), core.__dict__)
    exec(compile(src[1], "<variant of %s: %r>" % (model.__name__, change), "exec"), mod.__dict__)
    mod.core = core
    return mod
