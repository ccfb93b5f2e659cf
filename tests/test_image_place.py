"""CPU: the host side of image detection (csrc/slam/image_place.hpp) through its stand-alone program tests/cpp/image_place_host.cpp --
the median rank, the inside test at the border, c = 7 against c = 8, a point behind the camera, the axes and their handedness -- and the
public surface: the headers declare the stages and the system entry points, alva::System's methods compile, the library exports them."""
import re
import subprocess
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("alva_image_match", "alva_image_homography", "alva_system_add_image", "alva_system_remove_image", "alva_system_reset_images",
         "alva_system_detect_images", "alva_system_debug_detect_images")


def test_image_placement_on_the_host(tmp_path):
    exe = tmp_path / "image_place_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(ROOT / "tests" / "cpp" / "image_place_host.cpp")])
    out = subprocess.run([str(exe)], text=True, capture_output=True)
    assert out.returncode == 0 and re.fullmatch(r"\d+ 0 failures", out.stdout.strip()), out.stdout


def test_headers_declare_image_detection():
    hip = (ROOT / "include" / "alvaar_hip.h").read_text()
    sysh = (ROOT / "include" / "alvaar_system.h").read_text()
    for name in ("image_match", "image_homography"):
        assert re.search(r"\bint\s+alva_%s\s*\(\s*alva_ctx\s*\*" % name, hip), name
    for name in ("add_image", "remove_image", "reset_images", "detect_images"):
        assert re.search(r"\bint\s+alva_system_%s\s*\(\s*alva_system\s*\*" % name, sysh), name
    assert re.search(r"\bint\s+alva_system_debug_detect_images\s*\(\s*alva_system\s*\*", sysh)   # beside alva_system_debug_light
    assert "the lowest row on ties" in hip and "the lowest `it` on ties" in hip   # the tie rules are part of the definition


def test_system_class_image_methods_compile():
    src = r'''
#include "alvaar_system.h"
int use(alva::System &s, const uint8_t *gray, int *ids, float *poses, float *extents, float *scale, float *quads, int *info) {
    const int id = s.addImage(gray, 256, 192, 256, 0.21);
    const int found = s.detectImages(256, 3.0f, 20, 8, ids, poses, extents, scale, quads, info);
    return id + found + s.removeImage(id) + s.resetImages();
}
'''
    with tempfile.TemporaryDirectory() as d:
        f = Path(d) / "t.cpp"
        f.write_text(src)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-fsyntax-only", str(f)])


def test_library_exports_image_detection():
    import ctypes
    lib = ctypes.CDLL(str(ROOT / "alvaar_amd" / "libalvaar_hip.so"))
    assert all(hasattr(lib, name) for name in NAMES)
