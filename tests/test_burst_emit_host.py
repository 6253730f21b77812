"""common.h's burst_emit and split Philox block on the HOST, without a device: the two pieces of text are cut out of the header, compiled as a
stand-alone program with the address and undefined-behaviour sanitizers, and run against what they replace -- burst_emit, lane by lane, against
the loops the four emitters had (same floats at the same addresses, guards on both sides untouched, no staged dword read outside [i0, i1));
philox_uniform + philox4x32_10_lane against philox4x32_10 over two million random counters and keys."""
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as G

COMMON = os.path.join(G.ROOT, "sorrel_amd", "csrc", "common.h")
PRELUDE = """#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define __device__
#define __forceinline__ inline
"""

BURST_MAIN = r"""
typedef float vfloat4 __attribute__((ext_vector_type(4)));
int main() {
    long cases = 0, bad = 0;
    // whole-env f32 burst: nd staged dwords, destination mis float4 behind a line
    for (int nd : {1, 3, 27, 56, 57, 63, 64, 65, 120, 127, 128, 129, 147, 441, 588, 640, 641}) for (int mis = 0; mis < 8; ++mis) {
        std::vector<uint32_t> ob(nd); for (auto& x : ob) x = (uint32_t)rand() * 2654435761u + rand();
        const int G = 256; std::vector<float> A(G + 4 * (nd + 8) + G, -9.f), B(A);
        float* oa = A.data() + G + 4 * mis; float* obb = B.data() + G + 4 * mis;
        for (int lane = 0; lane < 64; ++lane)   // the loop as it was
            for (int i = lane - mis; i < nd; i += 64) { if (i < 0) continue; uint32_t b = ob[i];
                oa[4*i] = (float)(b & 0xFFu); oa[4*i+1] = (float)((b >> 8) & 0xFFu); oa[4*i+2] = (float)((b >> 16) & 0xFFu); oa[4*i+3] = (float)(b >> 24); }
        const uint32_t* ob4 = ob.data();
        for (int lane = 0; lane < 64; ++lane)
            burst_emit<true>(reinterpret_cast<vfloat4*>(obb) - mis, mis, mis + nd, lane, [&](const int i) { if (i - mis < 0 || i - mis >= nd) { printf("OOB load\n"); exit(2); } return ob4[i - mis]; }, [](const uint32_t k) { return (float)k; });
        ++cases; if (memcmp(A.data(), B.data(), A.size() * 4)) { ++bad; printf("f32 nd %d mis %d differs\n", nd, mis); }
    }
    // u8 twin: dwords, mis < 32
    for (int nd : {1, 27, 31, 32, 33, 63, 64, 65, 147, 588}) for (int mis = 0; mis < 32; ++mis) {
        std::vector<uint32_t> ob(nd); for (auto& x : ob) x = (uint32_t)rand() * 2654435761u + rand();
        const int G = 128; std::vector<uint32_t> A(G + nd + 32 + G, 0xA5A5A5A5u), B(A);
        uint32_t* oa = A.data() + G + mis; uint32_t* obb = B.data() + G + mis;
        for (int lane = 0; lane < 64; ++lane) for (int i = lane; i < nd; i += 64) oa[i] = ob[i];
        const uint32_t* ob4 = ob.data();
        for (int lane = 0; lane < 64; ++lane)
            burst_emit<false>(obb - mis, mis, mis + nd, lane, [&](const int i) { if (i - mis < 0 || i - mis >= nd) { printf("OOB load\n"); exit(2); } return ob4[i - mis]; }, [](const uint32_t k) { return (float)k; });
        ++cases; if (memcmp(A.data(), B.data(), A.size() * 4)) { ++bad; printf("u8 nd %d mis %d differs\n", nd, mis); }
    }
    // emit_chunk's interior: dwords [i0, i1) of the staging area, any pair (i1 < i0 included)
    for (int i0 = 0; i0 <= 9; ++i0) for (int i1 = 0; i1 < 400; ++i1) {
        std::vector<uint32_t> ob(512); for (auto& x : ob) x = (uint32_t)rand() * 2654435761u + rand();
        const int G = 64; std::vector<float> A(G + 4 * 512 + G, -9.f), B(A);
        float* ga = A.data() + G; float* gb = B.data() + G;
        for (int lane = 0; lane < 64; ++lane) for (int i = lane; i < i1; i += 64) { if (i < i0) continue; uint32_t b = ob[i];
            ga[4*i] = (float)(b & 0xFFu); ga[4*i+1] = (float)((b >> 8) & 0xFFu); ga[4*i+2] = (float)((b >> 16) & 0xFFu); ga[4*i+3] = (float)(b >> 24); }
        for (int lane = 0; lane < 64; ++lane)
            burst_emit<true>(gb, i0, i1, lane, [&](const int i) { if (i < i0 || i >= i1) { printf("OOB load\n"); exit(2); } return ob[i]; }, [](const uint32_t k) { return (float)k; });
        ++cases; if (memcmp(A.data(), B.data(), A.size() * 4)) { ++bad; printf("chunk %d %d differs\n", i0, i1); }
    }
    // a first iteration beyond dword 64 (k0 > 0)
    for (int i0 : {64, 65, 100, 127, 128, 130}) for (int i1 : {64, 66, 128, 129, 191, 192, 193, 300}) {
        std::vector<uint32_t> ob(512, 0x01020304u); const int G = 64; std::vector<float> A(G + 4 * 512 + G, -9.f), B(A);
        float* ga = A.data() + G; float* gb = B.data() + G;
        for (int i = i0; i < i1; ++i) { ga[4*i] = 4; ga[4*i+1] = 3; ga[4*i+2] = 2; ga[4*i+3] = 1; }
        for (int lane = 0; lane < 64; ++lane) burst_emit<true>(gb, i0, i1, lane, [&](const int i) { return ob[i]; }, [](const uint32_t k) { return (float)k; });
        ++cases; if (memcmp(A.data(), B.data(), A.size() * 4)) { ++bad; printf("late %d %d differs\n", i0, i1); }
    }
    printf("%ld cases, %ld differ\n", cases, bad);
    return bad != 0;
}
"""

PHILOX_MAIN = r"""
int main(){ unsigned long long bad=0; srand(1);
 for (int it=0; it<2000000; ++it){ uint32_t v[6]; for(int i=0;i<6;++i) v[i]=((uint32_t)rand()<<17)^((uint32_t)rand()<<3)^rand();
  if (it<64){ v[0]=it; } if (it%7==0) v[1]=it;
  U4 a=philox4x32_10<false>(v[0],v[1],v[2],v[3],v[4],v[5]);
  PhiloxUniform u=philox_uniform(v[1],v[2],v[3],v[4],v[5]);
  U4 b=philox4x32_10_lane<false>(v[0],u,v[4],v[5]);
  U4 c=philox4x32_10_lane<true>(v[0],u,v[4],v[5]);
  if(a.x!=b.x||a.y!=b.y||a.z!=b.z||a.w!=b.w||a.x!=c.x||a.w!=c.w) ++bad; }
 printf("mismatches %llu\n", bad); return bad!=0; }
"""


def _clang():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    if not os.path.isfile(clang):
        clang = shutil.which("clang++")
    if not clang:
        pytest.fail("no clang++ (the helper uses ext_vector_type): the host check cannot be built")
    return clang


def _cut(text, first, last):
    return text[text.index(first):text.index(last)]


def _run(tmp_path, name, source):
    src = tmp_path / (name + ".cpp")
    src.write_text(source)
    exe = tmp_path / name
    out = subprocess.run([_clang(), "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    return out.stdout


def test_burst_emit_writes_what_the_old_loops_wrote(tmp_path):
    text = open(COMMON).read()
    body = _cut(text, "template <bool F32, class Load, class ToF>", "// ---------------------------------------------------------------- grid <-> LDS")
    assert body.count('asm volatile("" : "+v"(voff));') == 1
    body = body.replace('asm volatile("" : "+v"(voff));', "")                  # (a compiler barrier on the device, nothing else)
    body, n = re.subn(r"__builtin_nontemporal_store\((\w+), (reinterpret_cast<[^>]+>\([^)]*\))\);", r"*(\2) = \1;", body)
    assert n == 2, n
    out = _run(tmp_path, "burst", PRELUDE + body + BURST_MAIN)
    assert re.search(r"\d+ cases, 0 differ", out), out


def test_split_philox_block_equals_the_whole_one(tmp_path):
    text = open(COMMON).read()
    body = _cut(text, "struct U4 {", "__device__ __forceinline__ uint32_t word_of")
    body, n = re.subn(r'asm\("v_bitop3_b32[^;]*;', "d = a ^ b ^ k;", body)
    assert n == 1, n
    body = body.replace('asm volatile("" : "+s"(k0), "+s"(k1));', ";").replace('asm volatile("" : "+v"(v));', ";")
    assert "asm" not in body, "device-only text left in the host build"
    out = _run(tmp_path, "philox", PRELUDE + body + PHILOX_MAIN)
    assert "mismatches 0" in out, out
