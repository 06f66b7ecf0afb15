"""Host side of the index build surface (``index_factory`` / ``extract_index_ivf`` / ``IVFFlatHIP.add`` / the opt-in faiss shim):
everything here runs without a GPU -- the untrained object never touches the library, and the C calls are stubbed where a trained
state is needed."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKEL = os.path.join(ROOT, "tests", "skeleton")


@pytest.mark.parametrize("desc,nlist", [("IVF1,Flat", 1), ("IVF30,Flat", 30), ("IVF16000,Flat", 16000)])
def test_description_parsing_serves_ivf_flat(desc, nlist):
    from rvc_amd import ivf

    assert ivf.parse_description(desc) == nlist


@pytest.mark.parametrize("desc", ["IVF30,PQ128x4fs,RFlat", "Flat", "IVF,Flat", "IVF0,Flat", "ivf30,flat", " IVF30,Flat", "IVF30,Flat\n",
                                  "IVF30, Flat", "IVF-3,Flat", "IVF3.0,Flat", "HNSW32", "", None, 30])
def test_description_parsing_refuses_everything_else_and_names_what_is_served(desc):
    import rvc_amd

    with pytest.raises(ValueError, match="IVF<nlist>,Flat"):
        rvc_amd.index_factory(768, desc)


def test_untrained_object_attributes_and_nprobe_carry_over(monkeypatch):
    import rvc_amd
    from rvc_amd import _lib, ivf

    with pytest.raises(ValueError):
        rvc_amd.index_factory(770, "IVF4,Flat")  # d must be a multiple of 4
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.index_factory(768, "IVF4,Flat", device="cpu")  # no CPU fallback
    f = rvc_amd.index_factory(768, "IVF4,Flat")
    assert isinstance(f, rvc_amd.IVFFlatHIP) and rvc_amd.extract_index_ivf(f) is f
    assert (f.is_trained, f.ntotal, f.d, f.nlist, f.nprobe) == (False, 0, 768, 4, 1)
    rvc_amd.extract_index_ivf(f).nprobe = 3  # web.py:551-552, before training
    assert f.nprobe == 3
    with pytest.raises(rvc_amd.RvcmiError):
        f.nprobe = 0
    x = np.zeros((10, 768), np.float32)
    for call in (lambda: f.add(x), lambda: f.search(x, 8), lambda: rvc_amd.write_index(f, "/nonexistent/x.index"),
                 lambda: f.reconstruct_n(0, 0), lambda: f.blob(), lambda: f.centroids()):
        with pytest.raises(rvc_amd.RvcmiError, match="not trained"):
            call()
    with pytest.raises(rvc_amd.RvcmiError, match="at least nlist"):
        f.train(x[:3])
    with pytest.raises(ValueError):
        f.train(np.zeros((10, 256), np.float32))
    assert not f.is_trained
    with pytest.raises(TypeError):
        rvc_amd.extract_index_ivf(object())

    # the trained state, with the library stubbed: train() hands the sizes over and carries nprobe into the new handle
    calls = []

    class Stub:
        def rvcmi_ivf_train(self, d, n, x_, nlist, niter, seed, dev, obj, out):
            calls.append(("train", d, n, nlist, niter, seed))
            out._obj.value = 0x1234  # (`out` is the byref of the handle slot)
            return 0

        def rvcmi_ivf_set_nprobe(self, h, v):
            calls.append(("set_nprobe", h.value, v))
            return 0

        def rvcmi_ivf_nprobe(self, h):
            return 3

        def rvcmi_ivf_ntotal(self, h):
            return 0

        def rvcmi_ivf_destroy(self, h):
            calls.append(("destroy", h.value))
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: Stub())
    monkeypatch.setattr(ivf, "_idx", lambda dev: 0)
    f.train(x)
    assert f.is_trained and calls == [("train", 768, 10, 4, 10, 1234), ("set_nprobe", 0x1234, 3)]
    assert f.nprobe == 3 and f.ntotal == 0
    f.train(x)  # a second train is a no-op
    assert len(calls) == 2
    f.__del__()
    assert calls[-1] == ("destroy", 0x1234)


def test_every_handle_is_trained():
    import rvc_amd

    assert rvc_amd.IVFFlatHIP(C.c_void_p(None), "cuda:0").is_trained is True


def test_new_symbols_are_declared_in_the_header_and_bound():
    from rvc_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "rvcmi.h")).read()
    bound = {name: args for name, _res, args in _lib.SYMBOLS}
    for name, nargs in (("rvcmi_ivf_add", 5), ("rvcmi_ivf_train", 9)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M)
        assert m, name + " is not declared in include/rvcmi.h"
        assert len(m.group(1).split(",")) == nargs == len(bound[name])
    assert "#define RVCMI_VERSION 2" in hdr and _lib.RVCMI_VERSION == 2  # additive: the ABI version stays


def test_plain_install_still_refuses_index_factory_and_the_switch_serves_it(monkeypatch):
    import rvc_amd

    had_faiss = sys.modules.get("faiss")
    if had_faiss is None:
        try:
            import faiss  # noqa

            pytest.skip("a real faiss is installed: the shim forwards to it")
        except ImportError:
            pass
    else:
        pytest.skip("a real faiss is loaded: the shim forwards to it")

    def purge():
        for m in [m for m in sys.modules if m.split(".")[0] in ("rvc", "infer", "faiss")]:
            del sys.modules[m]

    purge()
    sys.path.insert(0, SKEL)
    try:
        monkeypatch.delenv("RVCMI_INDEX_BUILD", raising=False)
        rvc_amd.install()
        import infer.modules.vc.pipeline as pl

        for name in ("index_factory", "extract_index_ivf"):
            with pytest.raises(AttributeError, match="faiss is not installed"):
                getattr(pl.faiss, name)
        rvc_amd.uninstall()
        assert "faiss" not in sys.modules
        for how in ("argument", "environment"):
            purge()
            if how == "argument":
                rvc_amd.install(index_build=True)
            else:
                monkeypatch.setenv("RVCMI_INDEX_BUILD", "1")
                rvc_amd.install()
            import infer.modules.vc.pipeline as pl2

            f = pl2.faiss.index_factory(768, "IVF30,Flat")
            assert isinstance(f, rvc_amd.IVFFlatHIP) and not f.is_trained and (f.d, f.nlist) == (768, 30)
            assert pl2.faiss.extract_index_ivf(f) is f
            with pytest.raises(ValueError, match="IVF<nlist>,Flat"):
                pl2.faiss.index_factory(768, "IVF30,PQ128x4fs,RFlat")
            with pytest.raises(TypeError):
                pl2.faiss.extract_index_ivf(object())
            with pytest.raises(AttributeError, match="faiss is not installed"):
                pl2.faiss.IndexFlatL2  # everything else is as before
            rvc_amd.uninstall()
            assert "faiss" not in sys.modules
            monkeypatch.delenv("RVCMI_INDEX_BUILD", raising=False)
    finally:
        rvc_amd.uninstall()
        sys.path.remove(SKEL)
        purge()
