// mesh_stages.cpp -- the --mesh stage of the densify CLI (stages.h): a sequence
// of stages over one mesh that stays on the device until it is written.  Each
// stage allocates from the shared DeviceMaps, re-points the mesh at its result
// and returns its member of the report.
#include "stages.h"

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <sys/stat.h>

namespace {

struct DeviceMesh {
    dp_tsdf_options volume; // the lattice it was extracted from
    dp_mesh_vertex *verts = nullptr;
    int32_t *tris = nullptr; // three vertex numbers a triangle
    int64_t nv = 0, nt = 0;
    int64_t vcap = 0, tcap = 0;       // the counts as extracted: no stage returns more, so they size every buffer
    float *normals = nullptr;         // three floats a vertex, once normals() ran
    std::vector<float> host_normals;  // the same on the host, with --mesh-normals only

    dp_mesh_vertex *vertex_buffer(DeviceMaps &m, const char *who = "--mesh") const
    {
        return (dp_mesh_vertex *)m.bytes((size_t)vcap * sizeof(dp_mesh_vertex), who);
    }
    int32_t *triangle_buffer(DeviceMaps &m) const
    {
        return (int32_t *)m.bytes((size_t)tcap * 3 * sizeof(int32_t), "--mesh");
    }
};

// The volume is the patches' bounding box padded by the truncation; the voxel
// defaults to the box's longest side / --mesh-dim, the truncation to four voxels.
dp_tsdf_options volume_options(const Args &args, const std::vector<dp_patch> &kept)
{
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool any = false;
    for (const dp_patch &p : kept) {
        if (!(std::isfinite(p.pos[0]) && std::isfinite(p.pos[1]) && std::isfinite(p.pos[2])))
            continue;
        for (int a = 0; a < 3; ++a) {
            lo[a] = any ? std::min(lo[a], (double)p.pos[a]) : (double)p.pos[a];
            hi[a] = any ? std::max(hi[a], (double)p.pos[a]) : (double)p.pos[a];
        }
        any = true;
    }
    if (!any)
        throw std::runtime_error("--mesh: no patches to bound the volume");
    const double side = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
    const double voxel = args.mesh_voxel > 0.0 ? args.mesh_voxel : side / args.mesh_dim;
    if (!(voxel > 0.0))
        throw std::runtime_error("--mesh: the patches have no extent (give --mesh-voxel)");
    const double trunc = args.mesh_trunc > 0.0 ? args.mesh_trunc : 4.0 * voxel;
    dp_tsdf_options to;
    dp_default_tsdf_options(&to);
    to.voxel = (float)voxel;
    to.trunc = (float)trunc;
    to.min_weight = args.mesh_min_weight;
    for (int a = 0; a < 3; ++a) {
        to.origin[a] = (float)(lo[a] - trunc);
        to.dim[a] = (int32_t)std::min(std::max(std::ceil((hi[a] - lo[a] + 2.0 * trunc) / voxel), 2.0), 1024.0);
    }
    return to;
}

// the maps integrated into the volume (dp_tsdf_integrate_device) and the volume
// meshed (dp_tsdf_mesh_device, once for the counts and once into buffers of that size)
JsonObject integrate_and_mesh(dp_ctx *ctx, int32_t V, DeviceMaps &m, DeviceMesh &mesh)
{
    const dp_tsdf_options &to = mesh.volume;
    const size_t points = (size_t)to.dim[0] * to.dim[1] * to.dim[2];
    float *d_tsdf = (float *)m.bytes(points * 4, "--mesh");
    int32_t *d_weight = (int32_t *)m.bytes(points * 4, "--mesh");
    uint32_t *d_rgb = (uint32_t *)m.bytes(points * 4, "--mesh");
    dp_tsdf_stats ts;
    check(ctx,
          dp_tsdf_integrate_device(ctx, m.vid.data(), V, &to, m.depth.data(), d_tsdf, d_weight, d_rgb, &ts, nullptr),
          "dp_tsdf_integrate_device");
    dp_mesh_stats ms;
    check(ctx,
          dp_tsdf_mesh_device(ctx, &to, d_tsdf, d_weight, d_rgb, nullptr, 0, &mesh.vcap, nullptr, 0, &mesh.tcap, &ms,
                              nullptr),
          "dp_tsdf_mesh_device");
    mesh.verts = mesh.vertex_buffer(m);
    mesh.tris = mesh.triangle_buffer(m);
    check(ctx,
          dp_tsdf_mesh_device(ctx, &to, d_tsdf, d_weight, d_rgb, mesh.vcap ? mesh.verts : nullptr, mesh.vcap, &mesh.nv,
                              mesh.tcap ? mesh.tris : nullptr, mesh.tcap, &mesh.nt, &ms, nullptr),
          "dp_tsdf_mesh_device");
    if (mesh.nv != mesh.vcap || mesh.nt != mesh.tcap)
        throw std::runtime_error("--mesh: the counts changed between two runs");
    JsonObject o;
    o.ms("ms", ts.integrate_ms + ms.mesh_ms).array("dim", to.dim, 3).g9("voxel", to.voxel).g9("trunc", to.trunc);
    o.integer("observed_voxels", ts.observed_voxels).integer("active_cells", ms.active_cells);
    return o.ms("integrate_ms", ts.integrate_ms).ms("mesh_ms", ms.mesh_ms);
}

dp_mesh_clean_options clean_options(const Args &args)
{
    dp_mesh_clean_options mco;
    dp_default_mesh_clean_options(&mco);
    if (args.mesh_min_component >= 0)
        mco.min_triangles = args.mesh_min_component;
    if (args.mesh_min_component_frac >= 0.0)
        mco.min_fraction = (float)args.mesh_min_component_frac;
    if (args.mesh_keep_largest >= 0)
        mco.max_components = (int32_t)args.mesh_keep_largest;
    return mco;
}

// --mesh-min-component / -frac / --mesh-keep-largest: the small components
// dropped (dp_mesh_clean_device)
JsonObject clean(dp_ctx *ctx, const Args &args, DeviceMaps &m, DeviceMesh &mesh)
{
    const dp_mesh_clean_options mco = clean_options(args);
    const int64_t vcap = mesh.vcap, tcap = mesh.tcap; // the mesh is as extracted: nv = vcap, nt = tcap
    dp_mesh_vertex *d_verts = mesh.vertex_buffer(m);
    int32_t *d_tris = mesh.triangle_buffer(m);
    dp_mesh_clean_stats cs;
    check(ctx,
          dp_mesh_clean_device(ctx, &mco, vcap ? mesh.verts : nullptr, vcap, tcap ? mesh.tris : nullptr, tcap,
                               vcap ? d_verts : nullptr, vcap, &mesh.nv, tcap ? d_tris : nullptr, tcap, &mesh.nt,
                               nullptr, nullptr, &cs, nullptr),
          "dp_mesh_clean_device");
    if (mesh.nv > vcap || mesh.nt > tcap)
        throw std::runtime_error("--mesh: the clean-up returned more than it was given");
    mesh.verts = d_verts;
    mesh.tris = d_tris;
    JsonObject o;
    o.integer("vertices_in", cs.vertices_in).integer("triangles_in", cs.triangles_in);
    o.integer("invalid_triangles", cs.invalid_triangles).integer("unused_vertices", cs.unused_vertices);
    o.integer("components", cs.components).integer("largest_triangles", cs.largest_triangles);
    o.integer("components_kept", cs.components_kept).integer("vertices_out", cs.vertices_out);
    return o.integer("triangles_out", cs.triangles_out).ms("clean_ms", cs.clean_ms);
}

dp_mesh_smooth_options smooth_options(const Args &args)
{
    dp_mesh_smooth_options mso;
    dp_default_mesh_smooth_options(&mso);
    mso.iterations = args.mesh_smooth;
    if (args.mesh_smooth_lambda != 0.0)
        mso.lambda = (float)args.mesh_smooth_lambda;
    if (args.mesh_smooth_mu <= 0.0)
        mso.mu = (float)args.mesh_smooth_mu;
    if (args.mesh_smooth_free_boundary)
        mso.flags |= DP_SMOOTH_FREE_BOUNDARY;
    return mso;
}

// --mesh-smooth: the vertex positions relaxed (dp_mesh_smooth_device; the triangles stay)
JsonObject smooth(dp_ctx *ctx, const Args &args, DeviceMaps &m, DeviceMesh &mesh)
{
    const dp_mesh_smooth_options mso = smooth_options(args);
    dp_mesh_vertex *d_verts = mesh.vertex_buffer(m);
    dp_mesh_smooth_stats ss;
    check(ctx,
          dp_mesh_smooth_device(ctx, &mso, mesh.nv ? mesh.verts : nullptr, mesh.nv, mesh.nt ? mesh.tris : nullptr,
                                mesh.nt, mesh.nv ? d_verts : nullptr, &ss, nullptr),
          "dp_mesh_smooth_device");
    mesh.verts = d_verts;
    JsonObject o;
    o.integer("steps", ss.steps).integer("movable_vertices", ss.movable_vertices);
    o.integer("pinned_vertices", ss.pinned_vertices).integer("isolated_vertices", ss.isolated_vertices);
    o.integer("edges", ss.edges).integer("boundary_edges", ss.boundary_edges);
    o.integer("nonmanifold_edges", ss.nonmanifold_edges).integer("max_valence", ss.max_valence);
    return o.ms("adjacency_ms", ss.adjacency_ms).ms("smooth_ms", ss.smooth_ms);
}

// cluster cell = F x the volume's voxel, the lattice anchored at the volume's origin
dp_mesh_decimate_options decimate_options(const Args &args, const dp_tsdf_options &volume)
{
    dp_mesh_decimate_options mdo;
    dp_default_mesh_decimate_options(&mdo);
    for (int a = 0; a < 3; ++a)
        mdo.origin[a] = volume.origin[a];
    mdo.cell = (float)(args.mesh_decimate * (double)volume.voxel);
    mdo.mode = args.mesh_decimate_quadric ? DP_DECIMATE_QUADRIC : DP_DECIMATE_MEAN;
    return mdo;
}

// --mesh-decimate: the vertices of every cell merged (dp_mesh_decimate_device)
JsonObject decimate(dp_ctx *ctx, const Args &args, DeviceMaps &m, DeviceMesh &mesh)
{
    const dp_mesh_decimate_options mdo = decimate_options(args, mesh.volume);
    dp_mesh_vertex *d_verts = mesh.vertex_buffer(m);
    int32_t *d_tris = mesh.triangle_buffer(m);
    dp_mesh_decimate_stats ds;
    int64_t dv = 0, dt = 0;
    check(ctx,
          dp_mesh_decimate_device(ctx, &mdo, mesh.nv ? mesh.verts : nullptr, mesh.nv, mesh.nt ? mesh.tris : nullptr,
                                  mesh.nt, mesh.vcap ? d_verts : nullptr, mesh.vcap, &dv, mesh.tcap ? d_tris : nullptr,
                                  mesh.tcap, &dt, nullptr, nullptr, &ds, nullptr),
          "dp_mesh_decimate_device");
    if (dv > mesh.nv || dt > mesh.nt)
        throw std::runtime_error("--mesh: the simplification returned more than it was given");
    mesh.nv = dv;
    mesh.nt = dt;
    mesh.verts = d_verts;
    mesh.tris = d_tris;
    JsonObject o;
    o.g9("cell", mdo.cell).boolean("quadric", args.mesh_decimate_quadric);
    o.integer("vertices_in", ds.vertices_in).integer("triangles_in", ds.triangles_in);
    o.integer("invalid_triangles", ds.invalid_triangles).integer("degenerate_triangles", ds.degenerate_triangles);
    o.integer("unused_vertices", ds.unused_vertices).integer("clamped_vertices", ds.clamped_vertices);
    o.integer("clusters", ds.clusters).integer("orphan_clusters", ds.orphan_clusters);
    o.integer("max_cluster", ds.max_cluster).integer("collapsed_triangles", ds.collapsed_triangles);
    o.integer("duplicate_triangles", ds.duplicate_triangles).integer("quadric_vertices", ds.quadric_vertices);
    o.integer("mean_vertices", ds.mean_vertices).integer("vertices_out", ds.vertices_out);
    return o.integer("triangles_out", ds.triangles_out).ms("decimate_ms", ds.decimate_ms);
}

// --mesh-normals: the normals of the mesh as it will be written
// (dp_mesh_normals_device); --mesh-colour weights the views by them, so it
// asks for them too, but they come to the host only to be written
JsonObject normals(dp_ctx *ctx, const Args &args, DeviceMaps &m, DeviceMesh &mesh)
{
    mesh.normals = (float *)m.bytes((size_t)mesh.vcap * 3 * sizeof(float), "--mesh");
    dp_mesh_normals_stats ns;
    check(ctx,
          dp_mesh_normals_device(ctx, mesh.nv ? mesh.verts : nullptr, mesh.nv, mesh.nt ? mesh.tris : nullptr, mesh.nt,
                                 mesh.nv ? mesh.normals : nullptr, &ns, nullptr),
          "dp_mesh_normals_device");
    mesh.host_normals.resize(args.mesh_normals ? (size_t)mesh.nv * 3 : 0);
    download(mesh.host_normals, mesh.normals, "--mesh: copy of the normals failed");
    JsonObject o;
    return o.integer("zero_normals", ns.zero_normals).ms("normals_ms", ns.normals_ms);
}

dp_mesh_render_options mesh_render_options(const Args &args)
{
    dp_mesh_render_options mro;
    dp_default_mesh_render_options(&mro);
    if (args.mesh_cull_back)
        mro.flags |= DP_MESH_RENDER_CULL_BACK;
    return mro;
}

// --mesh-depth-maps: the mesh as it will be written rendered into every view
// (dp_mesh_render_device) and the planes written as PFM files; --mesh-colour
// reads the same depth planes, rendered once for both
JsonObject render(dp_ctx *ctx, const Args &args, int32_t V, DeviceMaps &m, const DeviceMesh &mesh, Planes &planes)
{
    if (!args.mesh_depth_dir.empty() && mkdir(args.mesh_depth_dir.c_str(), 0777) != 0 && errno != EEXIST)
        throw std::runtime_error("cannot create " + args.mesh_depth_dir);
    const dp_mesh_render_options mro = mesh_render_options(args);
    planes = device_planes(ctx, args.level, V, args.mesh_depth_normals, m, "--mesh-depth-maps");
    dp_mesh_render_stats rs;
    check(ctx,
          dp_mesh_render_device(ctx, mesh.nv ? mesh.verts : nullptr, mesh.nv, mesh.nt ? mesh.tris : nullptr, mesh.nt,
                                m.vid.data(), V, &mro, planes.depth.data(), nullptr,
                                args.mesh_depth_normals ? planes.normal.data() : nullptr, &rs, nullptr),
          "dp_mesh_render_device");
    std::vector<float> plane;
    for (int32_t v = 0; v < V && !args.mesh_depth_dir.empty(); ++v) {
        const int w = planes.w[(size_t)v], h = planes.h[(size_t)v];
        const float *src[2] = {planes.depth[(size_t)v], planes.normal[(size_t)v]};
        const char *stem[2] = {"mesh_depth", "mesh_normal"};
        for (int j = 0; j < 2; ++j) {
            if (!src[j])
                continue;
            const int ch = j ? 3 : 1;
            plane.resize((size_t)w * h * ch);
            download(plane, src[j], "--mesh-depth-maps: copy of a plane failed");
            dpio::write_pfm(view_pfm(args.mesh_depth_dir, stem[j], v), plane.data(), w, h, ch);
        }
    }
    JsonObject o;
    o.integer("views", V).boolean("cull_back", args.mesh_cull_back).integer("triangles", rs.triangles);
    o.integer("invalid_triangles", rs.invalid_triangles).integer("pairs", rs.pairs);
    o.integer("clipped_pairs", rs.clipped_pairs).integer("culled_pairs", rs.culled_pairs);
    o.integer("pixel_tests", rs.pixel_tests).integer("covered_pixels", rs.covered_pixels);
    return o.ms("render_ms", rs.render_ms);
}

dp_mesh_colour_options colour_options(const Args &args)
{
    dp_mesh_colour_options mco;
    dp_default_mesh_colour_options(&mco);
    if (args.mesh_colour_tol >= 0.0)
        mco.depth_tol = (float)args.mesh_colour_tol;
    if (args.mesh_colour_min_cos >= 0.0)
        mco.min_cos = (float)args.mesh_colour_min_cos;
    if (args.mesh_colour_bilinear)
        mco.flags |= DP_MESH_COLOUR_BILINEAR;
    return mco;
}

// --mesh-colour: the vertices coloured by the views that see them
// (dp_mesh_colour_device over the rendered depth planes), the last stage
JsonObject colour(dp_ctx *ctx, const Args &args, int32_t V, DeviceMaps &m, DeviceMesh &mesh, const Planes &planes)
{
    const dp_mesh_colour_options mco = colour_options(args);
    dp_mesh_vertex *d_verts = mesh.vertex_buffer(m, "--mesh-colour");
    dp_mesh_colour_stats cs;
    check(ctx,
          dp_mesh_colour_device(ctx, mesh.nv ? mesh.verts : nullptr, mesh.nv, mesh.nv ? mesh.normals : nullptr,
                                m.vid.data(), V, &mco, planes.depth.data(), mesh.nv ? d_verts : nullptr, nullptr,
                                nullptr, &cs, nullptr),
          "dp_mesh_colour_device");
    mesh.verts = d_verts;
    JsonObject o;
    o.integer("views", V).boolean("bilinear", args.mesh_colour_bilinear);
    o.g9("depth_tol", mco.depth_tol).g9("min_cos", mco.min_cos).integer("vertices", cs.vertices);
    o.integer("projected_pairs", cs.projected_pairs).integer("occluded_pairs", cs.occluded_pairs);
    o.integer("grazing_pairs", cs.grazing_pairs).integer("visible_pairs", cs.visible_pairs);
    o.integer("coloured_vertices", cs.coloured_vertices).integer("unseen_vertices", cs.unseen_vertices);
    return o.ms("colour_ms", cs.colour_ms);
}

void download_and_write(const Args &args, const DeviceMesh &mesh)
{
    std::vector<dp_mesh_vertex> verts((size_t)mesh.nv);
    std::vector<int32_t> tris((size_t)mesh.nt * 3);
    download(verts, mesh.verts, "--mesh: copy of the mesh failed");
    download(tris, mesh.tris, "--mesh: copy of the mesh failed");
    std::vector<dpio::MeshPoint> out(verts.size());
    for (size_t i = 0; i < verts.size(); ++i)
        for (int k = 0; k < 3; ++k) {
            out[i].pos[k] = verts[i].pos[k];
            out[i].rgb[k] = verts[i].rgb[k];
        }
    dpio::write_mesh_ply(args.mesh_path, out, tris, args.mesh_normals ? &mesh.host_normals : nullptr);
}

} // namespace

void write_mesh(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept, Evaluation *ev,
                JsonObject &report)
{
    DeviceMesh mesh;
    mesh.volume = volume_options(args, kept);
    DeviceMaps m;
    render_device_maps(ctx, args, V, kept, "--mesh", m);
    // `inside` "mesh" go the stages that keep the triangles, beside it the others
    JsonObject inside = integrate_and_mesh(ctx, V, m, mesh), beside;
    if (args.mesh_clean())
        inside.object("clean", clean(ctx, args, m, mesh));
    if (args.mesh_smooth >= 0)
        inside.object("smooth", smooth(ctx, args, m, mesh));
    const DeviceMesh before = mesh; // what --mesh-decimate is given (--eval-mesh-surface)
    if (args.mesh_decimate > 0.0)
        beside.object("mesh_decimate", decimate(ctx, args, m, mesh));
    if (args.mesh_normals || args.mesh_colour)
        inside.object("normals", normals(ctx, args, m, mesh));
    Planes planes;
    if (!args.mesh_depth_dir.empty() || args.mesh_colour)
        beside.object("mesh_render", render(ctx, args, V, m, mesh, planes));
    if (args.mesh_colour)
        beside.object("mesh_colour", colour(ctx, args, V, m, mesh, planes));
    download_and_write(args, mesh);
    if (ev)
        ev->add("mesh_vertices", mesh.verts, mesh.nv, sizeof(dp_mesh_vertex));
    if (ev && args.eval_mesh_surface) {
        ev->add_mesh_surface(mesh.verts, mesh.nv, mesh.tris, mesh.nt);
        if (args.mesh_decimate > 0.0)
            ev->add_deviation("decimate_deviation", before.verts, before.nv, before.tris, before.nt, mesh.verts,
                              mesh.nv, mesh.tris, mesh.nt);
    }
    if (!m.refined.empty())
        report.object("mesh_refined", m.refined);
    JsonObject o;
    report.object("mesh", o.integer("vertices", mesh.nv).integer("triangles", mesh.nt).members(inside)).members(beside);
}
