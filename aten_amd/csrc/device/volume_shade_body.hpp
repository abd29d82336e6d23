// The body of the volume renderer's shade kernel: VolumePathTracing::Nee (volume_pathtracing.cpp:228-407) + ShadeMiss with
// bounce = depth_count + the bookkeeping of TraverseShadowRay (volume_pathtracing_impl.h:285-293), one path per lane over the
// iteration's queue.  Included twice as text, so that the gridless kernel is compiled from exactly the statements it always had:
//   ATN_VOL_SHADE_GRID 0  k_vol_shade<MS>       (device/volume.hpp; pb, sc, fp, cam, va, it)
//   ATN_VOL_SHADE_GRID 1  k_vol_shade_grid<MS>  (device/volume_grid.hpp; vg as well): a medium that names a grid is delta-tracked where
//                         the homogeneous free flight is sampled, and a connection record gets a sample stream of its own
    __shared__ BlockAppendShared sh;
    const uint32_t count = va.counters[kVolCntQueue + it];
    const uint32_t* __restrict__ q = pb.queue[it & 1];
    uint32_t* qn = pb.queue[(it + 1) & 1];
    for (uint32_t j0 = blockIdx.x * 256u; j0 < count; j0 += gridDim.x * 256u) {
        const uint32_t j = j0 + threadIdx.x;
        bool push_next = false, push_conn = false;
        uint32_t slot = 0u;
        if (j < count) {
            slot = q[j];
            const float4 ro4 = pb.ray_o[slot], rd4 = pb.ray_d[slot];
            f3 ray_org = mk3(ro4);
            const f3 ray_dir = mk3(rd4);
            float pdfb = ro4.w;
            uint32_t flags = __float_as_uint(rd4.w) & ~F_HIT;
            const float4 is4 = pb.isect[slot];
            const int32_t hit_objid = __float_as_int(is4.x);
            const float4 thr4 = pb.thr[slot];
            f3 throughput = mk3(thr4);
            uint32_t meta = va.meta[slot];
            VolStack st = vol_stack_load(va.stack[slot], meta);
            int32_t depth = (int32_t)((meta >> 4) & 255u);
            bool sh_active = ((meta >> 12) & 1u) != 0u;
            int32_t px = 0, py = 0;
            slot_to_pixel(fp, slot, px, py);
            const uint32_t pixel = (uint32_t)(py * fp.width + px);
            Cmj smp;
            {
                const uint32_t fs = fp.frame + (uint32_t)fp.sample;
                const uint32_t rnd = pb.seeds[pixel < fp.n_seeds ? pixel : pixel % fp.n_seeds];
                smp.idx = fs % 256u; smp.dim = __float_as_uint(thr4.w); smp.scramble = rnd * 0x1fe3434fu * ((fs + 133u * rnd) / 256u);
            }
            const bool cap = va.capture == it && fp.sample == 0;
            const uint32_t pixel_bits = pixel | (cap ? 0x80000000u : 0u);
            uint32_t sflags = kVolProcessed;
            float s_dist = 0.0F;
            f3 next_o = ray_org, next_d = ray_dir;
            bool new_ray = false;
            f3 contrib_add = mk3(0.0F);
            bool contrib_changed = false;
#if ATN_VOL_SHADE_GRID
            uint32_t conn_dim = 0u;      // the path's dimension at the moment the connection record is written
#endif

            if (hit_objid < 0) {
                // ---------------- ShadeMiss (pathtracing_impl.h:112-175), bounce = depth_count
                f3 dir = ray_dir;
                if (depth == 0) {
                    const float s = (float)px / (float)fp.width;
                    const float t = (float)py / (float)fp.height;
                    f3 o;
                    pinhole_sample(cam, s, t, o, dir);
                }
                const float4 emit = background_sample(sc, dir);
                float misW = 1.0f;
                if (!(depth == 0 || (depth == 1 && (flags & F_SINGULAR)))) {
                    float pdfLight = luminance(emit.x, emit.y, emit.z) / sc.avgIllum;
                    pdfLight /= (2.0f * kPi);
                    if (sc.ibl_importance) pdfLight = ibl_direction_pdf(sc, dir);
                    misW = pdfb / (pdfLight + pdfb);
                }
                f3 c = 1.0F * mk3(mul4(misW, emit)) + mk3(0.0F);
                c = c * throughput;
                contrib_add = c; contrib_changed = true;
                flags |= F_TERMINATED;
            }
            else {
                flags |= F_HIT;
                sflags |= kVolHit;
                const float hit_t = va.hit_t[slot];
                // ---- ComputeRussianProbability on depth_count
                float russian_prob = 1.0f;
                if (depth > fp.rr_depth) {
                    if (dot(throughput, throughput) > 0) {
                        russian_prob = max3(throughput);
                        const float p = cmj_next(smp);
                        if (p >= russian_prob) flags |= F_TERMINATED; else flags &= ~F_TERMINATED;
                    }
                }
                bool will_update_depth = false;
                if (flags & F_TERMINATED) {
                    // Nee returns before it clears the shadow ray: TraverseShadowRay connects the LAST event's point again
                    if (sh_active) {
                        const float4 eo = va.ev_o[slot], ed = va.ev_d[slot];
                        push_conn = vol_event_connection(sc, va, slot, pixel_bits, smp, mk3(eo), mk3(ed), throughput, st);
#if ATN_VOL_SHADE_GRID
                        conn_dim = smp.dim;
#endif
                    }
                }
                else {
                    throughput = throughput / russian_prob;
                    const int32_t tri_id = __float_as_int(is4.w);
                    HitRec rec;
                    evaluate_hit(rec, sc, hit_objid, tri_id, is4.y, is4.z);
                    const int32_t mtrlid = triangle_mtrlid(sc, tri_id);
                    const int32_t mtrl_slot = mtrlid >= 0 ? mtrlid : sc.n_materials;
                    const DevMaterial& m = sc.materials[mtrl_slot];
                    const uint32_t mflags = va.med[mtrl_slot].flags;
                    const bool isBackfacing = dot(rec.normal, -ray_dir) < 0.0F;
                    f3 orienting_normal = rec.normal;
                    sh_active = false;
                    bool is_scattered = false;
                    f3 ev_dir = ray_dir;
#if ATN_VOL_SHADE_GRID
                    bool in_grid = false;
                    {
                        if (st.n > 0u && (va.med[st.bottom].flags & kVolGridFlag)) {
                            // ---- HeterogeneousMedium::Sample, medium.cpp:58-151: the flight ends at min(box exit, hit distance)
                            in_grid = true;
                            const VolMedium md = va.med[st.bottom];
                            const atn_vg::Grid g = vg.grids[md.flags >> kVolGridShift];
                            VolDraw draw{ smp };
                            atn_vg::NoTie tie;
                            uint32_t steps = 0u;
                            float factor = 1.0F, le_factor = 1.0F;
                            const int ev = atn_vg::delta_track(g, md.sigma_a, md.sigma_s, md.sigma_t, ray_org.x, ray_org.y, ray_org.z, ray_dir.x, ray_dir.y, ray_dir.z,
                                                               hit_t, draw, tie, s_dist, steps, factor, le_factor);
                            sflags |= steps << 16;
                            if (ev != atn_vg::kFlightMiss) {
                                sflags |= kVolSampled;
                                ray_org = ray_org + ray_dir * s_dist;
                            }
                            if (ev == atn_vg::kFlightCapped) atomicAdd(&va.counters[kVolCntFrame + 4], 1u);
                            if (ev == atn_vg::kFlightScatter) {
                                const float r3 = cmj_next(smp);
                                const float r4 = cmj_next(smp);
                                ev_dir = normalize(hg_sample(r3, r4, md.g, -ray_dir));
                                throughput = throughput * factor;
                                sflags |= kVolScattered;
                                is_scattered = true;
                                sh_active = true;
                                va.ev_o[slot] = make_float4(ray_org.x, ray_org.y, ray_org.z, 0.0F);
                                va.ev_d[slot] = make_float4(ev_dir.x, ev_dir.y, ev_dir.z, 0.0F);
                            }
                        }
                    }
                    if (st.n > 0u && !in_grid) {
#else
                    if (st.n > 0u) {
#endif
                        // ---- HomogeniousMedium::Sample, medium.h:26-83
                        const VolMedium md = va.med[st.bottom];
                        const float sigma_t = md.sigma_a + md.sigma_s;
                        const float r1 = cmj_next(smp);
                        // the logarithm in double, rounded once (as the host library's logf evaluates it): at most 1 ulp from the twin's,
                        // so s stays within 2 ulp behind the division by ANY sigma_t.  With logf (<= 1 ulp, but on the other side of
                        // the true value at times) the two logarithms lay up to 2 ulp apart, and a sigma_t that is no power of two
                        // turned that into 3 ulp of s (docs/VOLUME.md, "Parity")
                        const float s = -(float)log((double)smax(1.0F - r1, 0.0F)) / sigma_t;
                        s_dist = s;
                        sflags |= kVolSampled;
                        if (s >= hit_t) ray_org = ray_org + ray_dir * hit_t;
                        else {
                            const float r2 = cmj_next(smp);
                            const float Pa = md.sigma_a / sigma_t;
                            ray_org = ray_org + ray_dir * s;
                            if (r2 < Pa) { throughput = throughput * mk3(md.le[0], md.le[1], md.le[2]); sflags |= kVolAbsorbed; }
                            else {
                                const float r3 = cmj_next(smp);
                                const float r4 = cmj_next(smp);
                                ev_dir = normalize(hg_sample(r3, r4, md.g, -ray_dir));
                                sflags |= kVolScattered;
                            }
                            is_scattered = true;
                            sh_active = true;
                            va.ev_o[slot] = make_float4(ray_org.x, ray_org.y, ray_org.z, 0.0F);
                            va.ev_d[slot] = make_float4(ev_dir.x, ev_dir.y, ev_dir.z, 0.0F);
                        }
                    }
                    bool is_reflected_or_refracted = false;
                    if (is_scattered) { next_o = ray_org; next_d = ev_dir; new_ray = true; }
                    else if ((m.attrib & ATN_MTRL_ATTR_EMISSIVE) && !isBackfacing) {
                        // ---- HitImplicitLight, pathtracing_impl.h:395-451 (ray.org is the hit point after a free flight without event)
                        const int32_t lid = sc.objects[hit_objid].light_id;
                        const f3 light_color = (lid >= 0 && lid < sc.n_lights) ? area_light_color(sc.lights[lid], rec.area) : mk3(0.0F);
                        float weight = 1.0f;
                        if (depth > 0) {
                            const float cosLight = dot(rec.normal, -ray_dir);
                            const f3 dv = rec.p - ray_org;
                            const float dist2 = dot(dv, dv);
                            if (cosLight >= 0) {
                                float pdfLight = 1 / rec.area;
                                pdfLight = (pdfLight * dist2) / cosLight;
                                weight = pdfb / (pdfb + pdfLight);
                            }
                        }
                        contrib_add = (throughput * weight) * light_color; contrib_changed = true;
                        flags |= F_TERMINATED;
                    }
                    else {
                        const VolStack st_before = st;
                        if ((mflags & (kVolMediumFlag | kVolPureFlag)) == (kVolMediumFlag | kVolPureFlag)) {
                            // a pure medium boundary: straight through
                            const f3 base = dot(ray_dir, orienting_normal) > 0 ? orienting_normal : -orienting_normal;
                            next_o = ray_offset(rec.p, base);
                            next_d = normalize(ray_dir);
                            new_ray = true;
                            sflags |= kVolPassed;
                        }
                        else {
                            const float4 albedo4 = sample_texture(sc, m.albedoMap, rec.u, rec.v, m.baseColor);
                            const f3 albedo = mk3(albedo4);
                            if (!(m.attrib & ATN_MTRL_ATTR_TRANSLUCENT) && isBackfacing) orienting_normal = -orienting_normal;
                            const float pre_r = apply_normal<MS>(sc, m, mtrl_slot, orienting_normal, rec.u, rec.v, ray_dir, smp);
                            // what the BSDF sample, the NEE evaluation and the light sample share at this vertex (shading.hpp, HitPre)
                            HitPre hp;
                            tangent_coordinate(orienting_normal, hp.t, hp.b);
                            hp.rough = ggx_roughness(sc, m, rec.u, rec.v);
                            hp.lambda_v = m.type == ATN_MTRL_GGX ? ggx_lambda(hp.rough, -ray_dir, orienting_normal) : 0.0F;
                            // ---- SampleLight + the connection record (the walk runs in k_vol_transmit: it draws nothing)
                            const bool invalid_mtrl = (m.attrib & (ATN_MTRL_ATTR_SINGULAR | ATN_MTRL_ATTR_TRANSLUCENT)) != 0;
                            if (sc.n_lights > 0 && !invalid_mtrl) {
                                int32_t li = (int32_t)(cmj_next(smp) * (float)sc.n_lights);
                                li = li < sc.n_lights - 1 ? li : sc.n_lights - 1;
                                LightSample ls;
                                ls.attrib = sc.lights[li].attrib;
                                sample_light(ls, sc.lights[li], sc, rec.p, orienting_normal, smp, &hp);
                                f3 radiance = mk3(0.0F);
                                const bool ok = radiance_nee_then<MS>(sc, ray_dir, orienting_normal, m, rec.u, rec.v, sc.inv_n_lights, ls, mtrl_slot, pre_r, nullptr,
                                                                      [&](const f3& r) { radiance = r; }, &hp);
                                const f3 nml = dot(ls.dir, orienting_normal) > 0 ? orienting_normal : -orienting_normal;
                                const f3 o = ray_offset(rec.p, nml);
                                const f3 d = normalize(ls.dir);
                                float dist = ls.dist;
                                if (ls.attrib & ATN_LIGHT_ATTR_INFINITE) dist = length(ls.pos - rec.p);
                                const float t_max = dist - va.eps_bias;
                                va.c_o[slot] = make_float4(o.x, o.y, o.z, t_max);
                                va.c_d[slot] = make_float4(d.x, d.y, d.z, __uint_as_float(kVolConnSurface | (ok ? 0u : kVolConnNoAdd)));
                                va.c_w[slot] = make_float4(1.0F, __uint_as_float(pixel_bits), __uint_as_float(vol_stack_meta(st)), __uint_as_float(0u));
                                va.c_a[slot] = make_float4(throughput.x, throughput.y, throughput.z, 0.0F);
                                va.c_b[slot] = make_float4(radiance.x, radiance.y, radiance.z, 0.0F);
                                va.c_c[slot] = make_float4(albedo.x, albedo.y, albedo.z, 0.0F);
                                va.c_stack[slot] = st.q;
                                if (cap && va.st_conn) {
                                    float4* so = va.st_conn + 3u * (size_t)pixel;
                                    so[0] = make_float4(o.x, o.y, o.z, t_max);
                                    so[1] = make_float4(d.x, d.y, d.z, 1.0F);
                                }
                                push_conn = true;
#if ATN_VOL_SHADE_GRID
                                conn_dim = smp.dim;
#endif
                            }
                            // ---- sampleMaterial + PrepareForNextBounce (the roulette probability divides a second time, as written)
                            MtrlSample ms;
                            sample_material<MS>(ms, sc, m, orienting_normal, ray_dir, smp, rec.u, rec.v, mtrl_slot, pre_r, &hp);
                            const f3 ndir = normalize(ms.dir);
                            const f3 ray_along_normal = dot(orienting_normal, ndir) >= 0.0f ? orienting_normal : -orienting_normal;
                            const float c = dot(ray_along_normal, ndir);
                            if (ms.pdf > 0 && c > 0) {
                                throughput = throughput * ((((albedo * ms.bsdf) * c) / ms.pdf));
                                throughput = throughput / russian_prob;
                            }
                            else flags |= F_TERMINATED;
                            if (!(flags & F_TERMINATED)) {
                                pdfb = ms.pdf;
                                flags = (m.attrib & ATN_MTRL_ATTR_SINGULAR) ? (flags | F_SINGULAR) : (flags & ~F_SINGULAR);
                                next_o = ray_offset(rec.p, ray_along_normal);
                                next_d = normalize(ndir);
                                new_ray = true;
                            }
                            is_reflected_or_refracted = true;
                        }
                        (void)st_before;
                        // ---- UpdateMedium with the ray that goes on (rays[idx].dir)
                        if (!vol_update_medium(ray_dir, next_d, orienting_normal, mflags, (uint32_t)m.id, st)) atomicAdd(&va.counters[kVolCntFrame + 0], 1u);
                    }
                    will_update_depth = is_scattered || is_reflected_or_refracted;
                    // ---- TraverseShadowRay's connection of this iteration's event (the stack is the path's: an event leaves it alone)
                    if (is_scattered) push_conn = vol_event_connection(sc, va, slot, pixel_bits, smp, ray_org, ev_dir, throughput, st);
#if ATN_VOL_SHADE_GRID
                    if (is_scattered) conn_dim = smp.dim;
#endif
                }
                if (will_update_depth) depth += 1;
                if (depth > fp.max_depth) flags |= F_TERMINATED;
            }
            if (push_conn) sflags |= kVolConn;
#if ATN_VOL_SHADE_GRID
            if (push_conn) vg.c_smp[slot] = make_uint4(smp.idx, conn_dim, smp.scramble ^ 0x5bd1e995u, 0u);
#endif
            // radiance's loop ends a path after MedisumStackSize iterations
            if (!(flags & F_TERMINATED) && it + 1 >= kVolIterations) flags |= F_TERMINATED;
            push_next = !(flags & F_TERMINATED);
            if (new_ray) pb.ray_o[slot] = make_float4(next_o.x, next_o.y, next_o.z, pdfb);
            pb.ray_d[slot] = make_float4(next_d.x, next_d.y, next_d.z, __uint_as_float(flags));
            pb.thr[slot] = make_float4(throughput.x, throughput.y, throughput.z, __uint_as_float(smp.dim));
            meta = vol_stack_meta(st) | ((uint32_t)depth << 4) | (sh_active ? 1u << 12 : 0u);
            va.meta[slot] = meta;
            va.stack[slot] = st.q;
            if (contrib_changed) {
                const f3 contrib = mk3(pb.contrib[slot]) + contrib_add;
                pb.contrib[slot] = make_float4(contrib.x, contrib.y, contrib.z, 0.0F);
            }
            if (cap && va.st_state) {
                if (flags & F_TERMINATED) sflags |= kVolTerminated;
                va.st_state[pixel] = make_uint4(sflags, (uint32_t)depth, st.n, smp.dim);
                va.st_stack[pixel] = st.q;
                va.st_ray[2u * (size_t)pixel] = make_float4(next_o.x, next_o.y, next_o.z, s_dist);
                va.st_ray[2u * (size_t)pixel + 1u] = make_float4(next_d.x, next_d.y, next_d.z, hit_objid >= 0 ? va.hit_t[slot] : 0.0F);
            }
        }
        block_append2(sh, qn, &va.counters[kVolCntQueue + it + 1], push_next ? 1u : 0u, va.conn_q, &va.counters[kVolCntConn + it], push_conn ? 1u : 0u,
                      [&](int) { return slot; });
    }
