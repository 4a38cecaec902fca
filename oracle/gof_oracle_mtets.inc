// gof_oracle_mtets.inc -- TEST INFRASTRUCTURE, included by gof_oracle.cpp.
// Restates _unbatched_marching_tetrahedra (utils/tetmesh.py:47-138) on the CPU, including the
// 32 Mi-tet chunking of :55-95 (which only changes the ORDER of the faces: faces are emitted
// chunk by chunk, within a chunk all 1-triangle tets first, then the 2-triangle tets; the
// crossing edges are globally unique and sorted by (min id, max id) either way, because
// torch.unique(dim=0) returns sorted rows, :71, :110).

namespace {
const int mt_triangle_table[16][6] = {           // tetmesh.py:23-40
    {-1,-1,-1,-1,-1,-1},{1,0,2,-1,-1,-1},{4,0,3,-1,-1,-1},{1,4,2,1,3,4},
    {3,1,5,-1,-1,-1},{2,3,0,2,5,3},{1,4,0,1,5,4},{4,2,5,-1,-1,-1},
    {4,5,2,-1,-1,-1},{4,1,0,4,5,1},{3,2,0,3,5,2},{1,3,5,-1,-1,-1},
    {4,1,2,4,3,1},{3,0,4,-1,-1,-1},{2,0,1,-1,-1,-1},{-1,-1,-1,-1,-1,-1} };
const int mt_num_triangles[16] = { 0,1,1,2,1,2,2,1,1,2,2,1,2,1,1,0 };   // :42
const int mt_base_tet_edges[12] = { 0,1, 0,2, 0,3, 1,2, 1,3, 2,3 };    // :43
}

extern "C" int gofref_mtets(int64_t V, int64_t Tt, const int64_t* tets, const float* vertices, const float* sdf, const float* scales,
                            int64_t* num_edges, int64_t* num_faces,
                            int64_t* edge_ids, float* edge_pos, float* edge_sdf, float* edge_scales, int64_t* faces,
                            int64_t cap_edges, int64_t cap_faces, int64_t chunk_size_arg)
{
    (void)V;
    struct E { int64_t a, b; };
    std::vector<E> all;
    std::vector<int64_t> valid;       // valid tet ids
    std::vector<int> tetindex;
    for (int64_t t = 0; t < Tt; t++) {
        int occ[4], sum = 0;
        for (int k = 0; k < 4; k++) { occ[k] = sdf[tets[4 * t + k]] > 0; sum += occ[k]; }   // :98-100
        if (!(sum > 0 && sum < 4)) continue;                                             // :102
        valid.push_back(t);
        tetindex.push_back(occ[0] * 1 + occ[1] * 2 + occ[2] * 4 + occ[3] * 8);         // :123
        for (int e = 0; e < 6; e++) {
            int64_t a = tets[4 * t + mt_base_tet_edges[2 * e]], b = tets[4 * t + mt_base_tet_edges[2 * e + 1]];
            if (a > b) std::swap(a, b);                                                  // :107-108
            all.push_back(E{ a, b });
        }
    }
    std::vector<E> uniq = all;
    auto lt = [](const E& l, const E& r) { return l.a < r.a || (l.a == r.a && l.b < r.b); };
    std::sort(uniq.begin(), uniq.end(), lt);
    uniq.erase(std::unique(uniq.begin(), uniq.end(), [](const E& l, const E& r) { return l.a == r.a && l.b == r.b; }), uniq.end());
    // crossing edges (:113) and mapping unique -> crossing index or -1 (:114-116)
    std::vector<int64_t> mapping(uniq.size(), -1);
    int64_t ne = 0;
    for (size_t i = 0; i < uniq.size(); i++) {
        int s2 = (sdf[uniq[i].a] > 0) + (sdf[uniq[i].b] > 0);
        if (s2 == 1) mapping[i] = ne++;
    }
    int64_t nf = 0;
    for (int ti : tetindex) nf += mt_num_triangles[ti];
    *num_edges = ne; *num_faces = nf;
    if (!edge_ids) return GOF_OK;
    if (ne > cap_edges || nf > cap_faces) { g_err = "mtets: output capacity too small"; return GOF_E_INVALID; }
    for (size_t i = 0; i < uniq.size(); i++) {
        int64_t m = mapping[i];
        if (m < 0) continue;
        const int64_t ab[2] = { uniq[i].a, uniq[i].b };
        for (int k = 0; k < 2; k++) {
            edge_ids[2 * m + k] = ab[k];
            for (int c = 0; c < 3; c++) edge_pos[(2 * m + k) * 3 + c] = vertices[3 * ab[k] + c];
            edge_sdf[2 * m + k] = sdf[ab[k]];
            edge_scales[2 * m + k] = scales[ab[k]];
        }
    }
    // faces: chunk by chunk (:55-57: torch.chunk(tets, Tt // chunk + 1) when Tt > chunk)
    const int64_t chunk_size = chunk_size_arg > 0 ? chunk_size_arg : 32ll * 1024 * 1024;      // (:55; smaller only for the chunk tests)
    int64_t nchunks = 1, per = Tt;
    if (Tt > chunk_size) { nchunks = Tt / chunk_size + 1; per = (Tt + nchunks - 1) / nchunks; }
    int64_t fo = 0;
    size_t vi0 = 0;
    for (int64_t c = 0; c < nchunks; c++) {
        const int64_t t_end = std::min(Tt, (c + 1) * per);
        size_t vi1 = vi0;
        while (vi1 < valid.size() && valid[vi1] < t_end) vi1++;
        for (int pass = 1; pass <= 2; pass++)
            for (size_t vi = vi0; vi < vi1; vi++) {
                const int ti = tetindex[vi];
                if (mt_num_triangles[ti] != pass) continue;
                int64_t em[6];
                for (int e = 0; e < 6; e++) {
                    const E& ed = all[6 * vi + e];
                    size_t pos = std::lower_bound(uniq.begin(), uniq.end(), ed, lt) - uniq.begin();
                    em[e] = mapping[pos];
                }
                for (int k = 0; k < 3 * pass; k++) faces[3 * fo + k] = em[mt_triangle_table[ti][k]];
                fo += pass;
            }
        vi0 = vi1;
    }
    return GOF_OK;
}
