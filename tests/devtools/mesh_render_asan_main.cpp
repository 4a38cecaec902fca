// A stand-alone program over the host-side orchestration of csrc/mesh_render.hip (workspace carving, argument checks) for a sanitizer
// build on the CPU: link it against the emulated library built with tests/hipemu/build_emu.py --asan, with -fsanitize=address,undefined.
//   NF = 0, N = 0 views, and the refused inputs of DESIGN.md 3.20; every buffer is exactly as large as its query says.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/gof_hip.h"
#include "../../include/gof_mesh_hip.h"

#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, gof_last_error()); return 1; } } while (0)

int main()
{
    const int W = 16, H = 12, N = 2;
    const int64_t stride = (int64_t)W * H;
    std::vector<float> V = { 2, 2, 1, 14, 2, 1, 2, 10, 1, 8, 8, 2 };
    std::vector<int32_t> F = { 0, 1, 2, 1, 3, 2 };
    std::vector<uint8_t> col(16, 200);
    std::vector<GofRasterView> views(N);
    for (auto& v : views) {
        std::memset(&v, 0, sizeof(v));
        v.w2c[0] = v.w2c[5] = v.w2c[10] = 1.0;
        v.fx = v.fy = 1.0; v.znear = 0.01; v.zfar = 20.0; v.W = W; v.H = H;
    }
    GofShadeParams P;
    std::memset(&P, 0, sizeof(P));
    P.mode = GOF_SHADE_SHADED; P.ambient = 0.25;
    for (int c = 0; c < 3; c++) { P.base[c] = 0.8; P.background[c] = 1.0; }
    for (int64_t nf : { (int64_t)2, (int64_t)0 })
        for (int n : { N, 0 }) {
            const int64_t nv = 4;
            std::vector<char> ws_n(gof_mesh_vertex_normals_ws_bytes(nv, nf)), ws_fn(gof_mesh_face_normals_ws_bytes()), ws_f(gof_mesh_render_faces_ws_bytes(nf, n, stride)),
                ws_s(gof_mesh_shade_ws_bytes());
            std::vector<float> normals(3 * nv), fnormals(3 * nf + 1), depth(n * stride + 1), image(3 * n * stride + 1), bary(3 * n * stride + 1);
            std::vector<int32_t> face(n * stride + 1);
            EXPECT(gof_mesh_vertex_normals(nv, V.data(), nf, F.data(), normals.data(), ws_n.data(), ws_n.size(), nullptr) == GOF_OK);
            EXPECT(gof_mesh_face_normals(nv, V.data(), nf, F.data(), fnormals.data(), ws_fn.data(), ws_fn.size(), nullptr) == GOF_OK);
            EXPECT(gof_mesh_render_faces(nv, V.data(), nf, F.data(), n, views.data(), stride, depth.data(), face.data(), nullptr, ws_f.data(), ws_f.size(), nullptr) == GOF_OK);
            EXPECT(gof_mesh_shade(nv, V.data(), nf, F.data(), normals.data(), col.data(), n, views.data(), stride, face.data(), &P, image.data(), bary.data(), ws_s.data(),
                                  ws_s.size(), nullptr) == GOF_OK);
            if (nf && n) EXPECT(face[5 * W + 5] == 0 && depth[5 * W + 5] == 1.0f && std::fabs(normals[2]) == 1.0f);
            if (!nf && n) EXPECT(face[5 * W + 5] == -1 && image[5 * W + 5] == 1.0f && normals[2] == 1.0f);
            // refused: nothing may be touched, whatever the sizes
            std::vector<int32_t> bad = F;
            bad[4] = 4;
            if (nf) {
                EXPECT(gof_mesh_vertex_normals(nv, V.data(), nf, bad.data(), normals.data(), ws_n.data(), ws_n.size(), nullptr) == GOF_E_INVALID);
                EXPECT(gof_mesh_render_faces(nv, V.data(), nf, bad.data(), n, views.data(), stride, depth.data(), face.data(), nullptr, ws_f.data(), ws_f.size(), nullptr) == GOF_E_INVALID);
            }
            if (n) {
                std::vector<GofRasterView> wide = views;
                wide[n - 1].W = 20000;
                EXPECT(gof_mesh_render_faces(nv, V.data(), nf, F.data(), n, wide.data(), stride, depth.data(), face.data(), nullptr, ws_f.data(), ws_f.size(), nullptr) == GOF_E_INVALID);
                wide = views;
                wide[0].znear = 0.0;
                EXPECT(gof_mesh_shade(nv, V.data(), nf, F.data(), normals.data(), col.data(), n, wide.data(), stride, face.data(), &P, image.data(), bary.data(), ws_s.data(),
                                      ws_s.size(), nullptr) == GOF_E_INVALID);
            }
            GofShadeParams Q = P;
            Q.mode = GOF_SHADE_COLOR;
            EXPECT(gof_mesh_shade(nv, V.data(), nf, F.data(), normals.data(), nullptr, n, views.data(), stride, face.data(), &Q, image.data(), bary.data(), ws_s.data(), ws_s.size(),
                                  nullptr) == GOF_E_INVALID);
            Q = P; Q.mode = 4;
            EXPECT(gof_mesh_shade(nv, V.data(), nf, F.data(), normals.data(), col.data(), n, views.data(), stride, face.data(), &Q, image.data(), bary.data(), ws_s.data(), ws_s.size(),
                                  nullptr) == GOF_E_INVALID);
            Q = P; Q.ambient = NAN;
            EXPECT(gof_mesh_shade(nv, V.data(), nf, F.data(), normals.data(), col.data(), n, views.data(), stride, face.data(), &Q, image.data(), bary.data(), ws_s.data(), ws_s.size(),
                                  nullptr) == GOF_E_INVALID);
            EXPECT(gof_mesh_render_faces(nv, V.data(), nf, F.data(), n, views.data(), stride, depth.data(), face.data(), nullptr, ws_f.data(), ws_f.size() - 1, nullptr) == GOF_E_WORKSPACE);
        }
    EXPECT(gof_mesh_render_faces_ws_bytes(10, -1, 4) == 0 && gof_mesh_render_abi_version() == 4);
    std::printf("mesh_render host orchestration: ok\n");
    return 0;
}
