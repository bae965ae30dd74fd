"""sk_scan_counted_device_async without a GPU: the symbol, its place in capi.EXPORTS, the Python signature, the ABI version."""
import inspect

from sickle_amd import capi


def test_symbol_is_exported_and_listed():
    assert "sk_scan_counted_device_async" in capi.EXPORTS
    assert hasattr(capi.lib(), "sk_scan_counted_device_async")


def test_context_method_signature():
    sig = inspect.signature(capi.Context.scan_counted_device_async)
    assert list(sig.parameters) == ["self", "params", "qual_ptr", "out_ptr", "n_reads_bound", "n_reads_dev_ptr", "offsets_ptr",
                                    "seq_ptr", "max_read_len", "stream"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {"seq_ptr": None, "max_read_len": 0, "stream": None}


def test_abi_version_stays_2():
    assert capi.lib().sk_abi_version() == 2
