"""The host codecs (lz77-sss_amd/csrc/host_codec.cpp: decode, extract, last_error) on their own: the
file compiles with a plain host compiler, and tests/cpp/host_codec_check.cpp, linked against it
directly, runs clean under the address and undefined-behaviour sanitizers."""
from __future__ import annotations

import re
import subprocess

from conftest import PKG, ROOT

SRC = PKG / "csrc" / "host_codec.cpp"


def test_host_codec_is_pure_host_code(tmp_path):
    subprocess.run(["g++", "-std=c++20", "-Wall", "-Werror", "-c", str(SRC), "-o", str(tmp_path / "host_codec.o")],
                   check=True)
    for inc in re.findall(r"#\s*include\s+(\S+)", SRC.read_text()):  # the public header + the standard library
        assert inc == '"../../include/lz77sss.h"' or re.fullmatch(r"<[a-z_]+>", inc), inc


def test_host_codec_under_sanitizers(tmp_path):
    exe = tmp_path / "host_codec_check"
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "host_codec_check.cpp"), str(SRC),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env={})
    assert r.returncode == 0, r.stdout + r.stderr
