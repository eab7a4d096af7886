// mesh_driver.cpp -- a stand-alone program around frog_amd/csrc/host/mesh_io.cpp, which tests/test_mesh_io.py compiles with it
// under -fsanitize=address,undefined and runs over good, cut and corrupt mesh files: the readers must refuse or read, never
// touch memory they do not own.
//   mesh_driver out_dir file...
// Per file one line: "ok <points> <faces> <indices>" or "refused <status>".  A mesh that was read is written to out_dir in every
// format and read back; points and faces must come back exactly from .obj, .ply and .vtk (exit 2 otherwise), and the .stl must
// be readable (exit 3).
#include "frog_host.h"

#include <cstdio>
#include <cstring>
#include <string>

static bool equal_bytes(const void *a, const void *b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; }

static bool same(const frog_mesh &a, const frog_mesh &b)
{
    return a.n_points == b.n_points && a.n_faces == b.n_faces && a.face_ptr[a.n_faces] == b.face_ptr[b.n_faces] &&
           equal_bytes(a.xyz, b.xyz, 12 * (size_t)a.n_points) && equal_bytes(a.face_ptr, b.face_ptr, 4 * ((size_t)a.n_faces + 1)) &&
           equal_bytes(a.face_idx, b.face_idx, 4 * (size_t)a.face_ptr[a.n_faces]);
}

int main(int argc, char *argv[])
{
    if (argc < 2) return 1;
    const std::string out_dir = argv[1];
    for (int i = 2; i < argc; i++) {
        int status = -1;
        frog_mesh_file *f = frog_mesh_read(argv[i], &status);
        if (!f) {
            if (status == FROG_OK || !*frog_mesh_last_error()) return 4;           // a refusal has a status and a message
            printf("refused %d\n", status);
            continue;
        }
        frog_mesh m;
        frog_mesh_view(f, &m);
        printf("ok %u %u %u\n", m.n_points, m.n_faces, m.face_ptr[m.n_faces]);
        for (const char *ext : { ".obj", ".ply", ".vtk", ".stl", ".vtp" }) {
            const std::string path = out_dir + "/roundtrip" + ext;
            if (frog_mesh_write(path.c_str(), &m)) return 5;
            if (!strcmp(ext, ".vtp")) continue;
            frog_mesh_file *g = frog_mesh_read(path.c_str(), &status);
            if (!g) return 3;
            frog_mesh r;
            frog_mesh_view(g, &r);
            const bool exact = strcmp(ext, ".stl") != 0;
            // NaN coordinates have no text form that keeps their bits: only meshes whose points are finite are compared
            bool finite = true;
            for (size_t k = 0; k < 3 * (size_t)m.n_points; k++) finite = finite && m.xyz[k] - m.xyz[k] == 0;
            if (exact && finite && !same(m, r)) return 2;
            frog_mesh_free(g);
        }
        frog_mesh_free(f);
    }
    return 0;
}
