// Stand-alone host program for a sanitizer run of the host-side parsing and validation behind hmsg_read_ply and hmsg_restore_stage
// (holoagent_amd/csrc/hmsg_stage_files.h: no HIP in it, nothing else is linked).  scripts/stage_files_asan.sh and
// tests/test_stage_files_sanitized.py build it with -fsanitize=address,undefined and run it; nothing is loaded into Python and no GPU is
// involved.  It writes good and damaged PLY files into the directory given as argv[1] and checks what the reader makes of each:
// truncated headers and bodies, over-long header lines, vertex counts the file cannot hold, other formats.
// Exit status 0 = every expectation met and no sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../holoagent_amd/csrc/hmsg_stage_files.h"

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);        \
            ++failures;                                               \
        }                                                             \
    } while (0)

static std::string put(const std::string& dir, const char* name, const std::string& bytes) {
    const std::string path = dir + "/" + name;
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) {
        fprintf(stderr, "cannot write %s\n", path.c_str());
        ++failures;
        return path;
    }
    fwrite(bytes.data(), 1, bytes.size(), f);
    fclose(f);
    return path;
}

template <typename T>
static void append(std::string& s, T v) {
    s.append(reinterpret_cast<const char*>(&v), sizeof(T));
}

static int read(const std::string& path, bool want, long long* n, std::vector<double>* out) {
    std::string msg;
    *n = -7;
    const int rc = stage_read_ply(path, want, n, out, &msg);
    EXPECT((rc == STAGE_OK) == msg.empty());
    return rc;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <scratch dir>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const std::string head_d = "ply\nformat binary_little_endian 1.0\ncomment Created by Open3D\nelement vertex 3\nproperty double x\nproperty double y\n"
                               "property double z\nend_header\n";
    std::string body_d;
    for (int i = 0; i < 9; ++i) append(body_d, (double)i * 0.5 - 1.0);
    long long n = 0;
    std::vector<double> pts;
    // ---- files that load
    EXPECT(read(put(dir, "ok_double.ply", head_d + body_d), true, &n, &pts) == STAGE_OK && n == 3 && pts.size() == 9 && pts[0] == -1.0 && pts[8] == 3.0);
    EXPECT(read(put(dir, "ok_double.ply", head_d + body_d), false, &n, &pts) == STAGE_OK && n == 3);
    {   // float coordinates, colours behind them, a face element after the vertices, trailing bytes
        std::string s = "ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
                        "property uchar green\nproperty uchar blue\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n";
        for (int i = 0; i < 2; ++i) {
            for (int a = 0; a < 3; ++a) append(s, (float)(i * 3 + a) + 0.25f);
            s += "\x01\x02\x03";
        }
        s += std::string("\x03", 1) + std::string(12, '\0');
        EXPECT(read(put(dir, "ok_float_rgb.ply", s), true, &n, &pts) == STAGE_OK && n == 2 && pts.size() == 6 && pts[0] == 0.25 && pts[5] == 5.25);
    }
    EXPECT(read(put(dir, "ok_empty.ply", "ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty double x\nproperty double y\nproperty double z\nend_header\n"),
                true, &n, &pts) == STAGE_OK && n == 0 && pts.empty());
    // ---- truncated headers: cut after every byte of a good header
    for (size_t cut = 0; cut < head_d.size(); ++cut)
        EXPECT(read(put(dir, "cut_header.ply", head_d.substr(0, cut)), true, &n, &pts) == STAGE_INVALID);
    // ---- truncated bodies: every length short of the promise
    for (size_t cut = 0; cut < body_d.size(); cut += 5) {
        EXPECT(read(put(dir, "cut_body.ply", head_d + body_d.substr(0, cut)), true, &n, &pts) == STAGE_INVALID);
        EXPECT(read(put(dir, "cut_body.ply", head_d + body_d.substr(0, cut)), false, &n, &pts) == STAGE_INVALID);
    }
    // ---- over-long header lines (the line buffer holds 512 bytes): a comment, a property name, the vertex count
    for (size_t len : {510u, 511u, 512u, 513u, 1023u, 1024u, 70000u}) {
        std::string s = "ply\nformat binary_little_endian 1.0\ncomment " + std::string(len, 'c') + "\nelement vertex 3\nproperty double x\nproperty double y\n"
                        "property double z\nend_header\n" + body_d;
        const int rc = read(put(dir, "long_comment.ply", s), true, &n, &pts);
        EXPECT(rc == STAGE_INVALID || (rc == STAGE_OK && n == 3 && pts.size() == 9));          // (refused or read right, never misread)
        s = "ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty double " + std::string(len, 'x') + "\nproperty double x\nproperty double y\n"
            "property double z\nend_header\n" + body_d;
        EXPECT(read(put(dir, "long_property.ply", s), true, &n, &pts) != STAGE_OK || n == 3);
        s = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::string(len, '9') + "\nproperty double x\nproperty double y\nproperty double z\nend_header\n" + body_d;
        EXPECT(read(put(dir, "long_count.ply", s), true, &n, &pts) == STAGE_INVALID);
    }
    EXPECT(read(put(dir, "no_newline.ply", std::string(100000, 'p')), true, &n, &pts) == STAGE_INVALID);
    {   // a header that never ends
        std::string s = "ply\nformat binary_little_endian 1.0\nelement vertex 3\n";
        for (int i = 0; i < 10000; ++i) s += "property double x\n";
        EXPECT(read(put(dir, "endless.ply", s), true, &n, &pts) == STAGE_INVALID);
    }
    // ---- counts the file cannot hold, negative counts, no count
    for (const char* cnt : {"4", "1000000000", "9223372036854775807", "-1", "-9223372036854775808", "", "x3"}) {
        const std::string s = std::string("ply\nformat binary_little_endian 1.0\nelement vertex ") + cnt + "\nproperty double x\nproperty double y\nproperty double z\nend_header\n" + body_d;
        EXPECT(read(put(dir, "bad_count.ply", s), true, &n, &pts) == STAGE_INVALID);
        EXPECT(read(put(dir, "bad_count.ply", s), false, &n, &pts) == STAGE_INVALID);
    }
    EXPECT(read(put(dir, "no_props.ply", "ply\nformat binary_little_endian 1.0\nelement vertex 3\nend_header\n" + body_d), true, &n, &pts) == STAGE_INVALID);
    EXPECT(read(put(dir, "no_z.ply", "ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty double x\nproperty double y\nend_header\n" + body_d), true, &n, &pts) == STAGE_INVALID);
    // ---- what this reader does not read
    EXPECT(read(put(dir, "ascii.ply", "ply\nformat ascii 1.0\nelement vertex 1\nproperty double x\nproperty double y\nproperty double z\nend_header\n0 0 0\n"), true, &n, &pts) == STAGE_UNSUPPORTED);
    EXPECT(read(put(dir, "big_endian.ply", "ply\nformat binary_big_endian 1.0\nelement vertex 3\nproperty double x\nproperty double y\nproperty double z\nend_header\n" + body_d), true, &n, &pts) ==
           STAGE_UNSUPPORTED);
    EXPECT(read(put(dir, "list.ply", "ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty list uchar int k\nproperty double x\nproperty double y\nproperty double z\nend_header\n" + body_d),
                true, &n, &pts) == STAGE_UNSUPPORTED);
    EXPECT(read(put(dir, "int_xyz.ply", "ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty int x\nproperty int y\nproperty int z\nend_header\n" + std::string(12, '\0')), true, &n,
                &pts) == STAGE_UNSUPPORTED);
    EXPECT(read(dir + "/does_not_exist.ply", true, &n, &pts) == STAGE_INVALID);
    EXPECT(read(put(dir, "empty.ply", ""), true, &n, &pts) == STAGE_INVALID);
    // ---- the offset check of hmsg_restore_stage
    {
        std::string msg;
        const int64_t good[] = {0, 1, 1, 64, 64}, down[] = {0, 5, 4, 9}, start[] = {1, 2, 3}, neg[] = {0, -1, 3}, zero[] = {0};
        EXPECT(stage_check_offsets(good, 4, &msg) == STAGE_OK && msg.empty());
        EXPECT(stage_check_offsets(zero, 0, &msg) == STAGE_OK);
        EXPECT(stage_check_offsets(down, 3, &msg) == STAGE_INVALID && msg.find("instance 1") != std::string::npos);
        EXPECT(stage_check_offsets(start, 2, &msg) == STAGE_INVALID);
        EXPECT(stage_check_offsets(neg, 2, &msg) == STAGE_INVALID);
        EXPECT(stage_check_offsets(nullptr, 2, &msg) == STAGE_INVALID);
        EXPECT(stage_check_offsets(good, -1, &msg) == STAGE_INVALID);
    }
    if (failures) {
        fprintf(stderr, "stage_files_asan: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("stage_files_asan ok\n");
    return 0;
}
