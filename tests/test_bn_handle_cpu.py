"""_ParamStore.bnh (no GPU): the BatchNorm handle of a trunk, a downsample, the stem's and a conformer convolution-module BatchNorm aliases
exactly what p32 / g32 / st.bn[base] / st.buffers return, for the ReLU-trunk Model, the E2E and the DC-TCN module, and is built once."""
import pytest

from test_store_module_cpu import _dctcn, _lrs, _lrw

BUILD = {"lrw": _lrw, "lrs": _lrs, "dctcn": _dctcn}


@pytest.mark.parametrize("which", ["lrw", "lrs", "dctcn"])
def test_bn_handle_aliases_the_store(which):
    m = BUILD[which]()
    st = m.store()
    bases = [f"{m.trunk_name}.layer1.0.bn1", f"{m.trunk_name}.layer2.0.bn2", f"{m.trunk_name}.layer2.0.downsample.1", f"{m.stem_name}.1"]
    if which == "lrw":
        assert m.trunk_act == 1, "the ReLU trunk"
    if which == "lrs":
        bases.append("encoder.encoders.0.conv_module.norm")
    for base in bases:
        assert base in st.bn, base
        h = st.bnh(base)
        assert st.bnh(base) is h, f"{base}: two calls, two handles"
        want = dict(gamma=st.p32(f"{base}.weight"), beta=st.p32(f"{base}.bias"), dgamma=st.g32(f"{base}.weight"), dbeta=st.g32(f"{base}.bias"),
                    coef=st.bn[base]["coef"], mean=st.bn[base]["mean"], rstd=st.bn[base]["rstd"], running_mean=st.buffers[f"{base}.running_mean"],
                    running_var=st.buffers[f"{base}.running_var"], num_batches_tracked=st.buffers[f"{base}.num_batches_tracked"])
        assert set(want) | {"C", "base"} == set(h._fields)
        for field, t in want.items():
            got = getattr(h, field)
            assert (got.data_ptr(), got.numel(), got.dtype) == (t.data_ptr(), t.numel(), t.dtype), (base, field)
        assert h.C == h.gamma.numel() == h.mean.numel() and h.coef.numel() == 3 * h.C and h.base == base
        # the flat buffers, not copies: the master weight, its gradient and the running statistics are what the module itself holds
        assert h.gamma.data_ptr() == dict(m.named_parameters())[f"{base}.weight"].data_ptr()
        assert h.dgamma.data_ptr() == dict(m.named_parameters())[f"{base}.weight"].grad.data_ptr()
        assert h.running_var.data_ptr() == dict(m.named_buffers())[f"{base}.running_var"].data_ptr()
