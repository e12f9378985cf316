"""The SHA-256 message-block builders without a GPU.

reticulum_amd/csrc/sha256_device.h holds the one rule for the end of a SHA-256
message (where 0x80 goes, when a second block is needed, where the bit length
lies) and the fixed blocks of HMAC and HKDF, as plain C++.  They are built for
the host with address and undefined-behaviour sanitizers
(tests/sha256_host/pad_check.cpp, a stand-alone program run directly) and
compared block by block with padding made the obvious way: one-segment
messages of every length 0..200, every split of two-segment messages of
0..130 bytes, the prefixed form for 0..130, each after 0 and after 64 bytes;
every message in a heap buffer of exactly its size.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_block_builders_match_obvious_padding_and_stay_inside_the_message(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of sha256_device.h")
    exe = str(tmp_path / "pad_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "sha256_host", "pad_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out = r.stdout.split()
    assert out[0] == "ok" and len(out) == 2
    # at least one block per case: 201 + 131 * 132 / 2 + 2 * 131 cases after each of two priors
    assert int(out[1]) >= 2 * (201 + 131 * 132 // 2 + 2 * 131)


def test_the_rule_is_spelled_once():
    """No SHA-256 initial state, HMAC pad constant or length-word store outside the one header."""
    csrc = os.path.join(ROOT, "reticulum_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name == "sha256_device.h" or not name.endswith((".h", ".hip")):
            continue
        text = open(os.path.join(csrc, name)).read()
        for needle in ("0x6a09e667u,", "0x36363636", "0x5c5c5c5c", "(bits >> 32)"):
            assert needle not in text, (name, needle)
