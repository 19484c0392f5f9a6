"""aclhip_order_track_requests_device / aclhip_decompress_track_batch_rows at the C ABI: declared, exported, argument checks that
need no device, and the header still a plain C99 header (no GPU)."""
import os
import subprocess

from acl_amd import runtime
from test_capi_symbols import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aclhip_order_track_requests_device", "aclhip_decompress_track_batch_rows")


def test_header_declares_and_library_exports_both_entry_points():
    declared = declared_functions()
    lib = runtime.load_library()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in runtime.EXPORTED_SYMBOLS, name


def test_a_null_context_is_an_invalid_argument():
    lib = runtime.load_library()
    assert lib.aclhip_order_track_requests_device(None, None, None, None, 16, None, None, None, None, None, None) == runtime.ERROR_INVALID_ARGUMENT
    assert lib.aclhip_order_track_requests_device(None, None, None, None, 0, None, None, None, None, None, None) == runtime.ERROR_INVALID_ARGUMENT
    params = runtime.default_params()
    assert lib.aclhip_decompress_track_batch_rows(None, None, None, None, None, 16, params, None, None) == runtime.ERROR_INVALID_ARGUMENT
    assert lib.aclhip_decompress_track_batch_rows(None, None, None, None, None, 0, params, None, None) == runtime.ERROR_INVALID_ARGUMENT


def test_the_header_with_both_declarations_is_plain_c99(tmp_path):
    source = tmp_path / "track_order_abi.c"
    source.write_text(
        "#include <aclhip.h>\n"
        "#include <stddef.h>\n"
        "int main(void)\n"
        "{\n"
        "\taclhip_status (*order)(aclhip_context*, const aclhip_clip*, const float*, const uint32_t*, uint32_t, uint32_t*, aclhip_clip*, float*,\n"
        "\t\tuint32_t*, uint32_t*, void*) = aclhip_order_track_requests_device;\n"
        "\taclhip_status (*decode)(aclhip_context*, const aclhip_clip*, const float*, const uint32_t*, const uint32_t*, uint32_t,\n"
        "\t\tconst aclhip_decompress_params*, void*, void*) = aclhip_decompress_track_batch_rows;\n"
        "\taclhip_decompress_params params;\n"
        "\taclhip_default_params(&params);\n"
        "\tif (order(NULL, NULL, NULL, NULL, 4, NULL, NULL, NULL, NULL, NULL, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)\n"
        "\t\treturn 1;\n"
        "\tif (decode(NULL, NULL, NULL, NULL, NULL, 4, &params, NULL, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)\n"
        "\t\treturn 2;\n"
        "\treturn 0;\n"
        "}\n")
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "track_order_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(source),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    assert subprocess.run([str(binary)], timeout=120).returncode == 0
