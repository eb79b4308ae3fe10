// pt_scene_records.hpp — the records of the device-private scene layout that the host builds (pt_scene_layout.hpp) and the kernels read
// (pt_device.hpp, which describes the node / triangle / shading records beside them).  Plain structs over the vector types: host compilers take it too.
#pragma once
#include <hip/hip_vector_types.h>

namespace ptd {

constexpr int REF_EMPTY = (int)0x80000000;
constexpr int PRIM_NONE = -1;
constexpr int PRIM_ELLIPSOID = 0x40000000;

struct ObjRoot { float bmin[3]; float bmax[3]; int ref; int pad; };           // 32 B
struct EllipRec {                                                                // frag.glsl:606-631
    float c[3], st[3], r; int mat; int rotated; float rot[3]; float R[9]; float RB[9]; float pad[2];
};
struct MatRec {                                                                  // the mtl fields trace()/chooseRay()/directDiffuse() read
    float Kd[3], Ks[3], Ke[3], Tf[3]; float Tr, Ni, Density, Pm, Pr, Pc, Pcr, subsurface; int illum;
    float Ka[3], ssColor[3], ssRadius[3];                                        // only directDiffuse (frag.glsl:661-675)
    int hasMaps;                                                                 // any of the map_* below > -1
    int map_Ka, map_Kd, map_Ks, map_Ke, map_Tr, map_Pm, map_Pr, map_Pc, map_norm; // texture indices (mapMtl :210-225, :827); -1 = none
    int niCode;                                                                  // Ni as an entry of the scene's refraction-index dictionary (DevScene::ni8 / niTable)
};                                                                               // 41 dwords = 164 B
struct TexRec { const uchar4* data; int w, h; };                                 // one entry of the bindless table (binding 15), RGBA8 texels as uploaded

}  // namespace ptd
