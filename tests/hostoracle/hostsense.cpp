// hostsense.cpp -- CPU build of the sensor calls of include/nudge_hip.h (nh_sense_rays, nh_sense), the oracle of the GPU's kernels
// (tests/hostsense_util.py).
//   hs_sense_rays  the ray of every (sensor, beam): nudge_amd/csrc/nh_query.h's nh_q_sensor_pose / nh_q_sensor_ray, the arithmetic the device runs, over
//                  a batch; the body transforms are a plain array of nh_Transform, or null for a call without bodies
//   hs_sense       oracle.h's closest_hit over SweptRay on each of those rays -- the brute force nh_raycast's oracle is -- under layer words and a mask
//                  per SENSOR; the record goes to `hits` and its t / body / tag to the three channels, each of which may be null
// Both run on several threads.
#include "oracle.h"

namespace {

nh_Ray ray_of(const nh_Sensor& s, const nh_Beam& b, const nh_Transform* bodies, uint32_t nbodies) {
	const bool mounted = bodies && s.body != 0xffffffffu;
	const bool exists = !mounted || s.body < nbodies;
	nh_f3 bp = nh_make3(0.0f, 0.0f, 0.0f);
	nh_quat bq = { 0.0f, 0.0f, 0.0f, 0.0f };
	if (mounted && exists) { bp = v3(bodies[s.body].position); bq = q4(bodies[s.body].rotation); }
	const nh_QPose w = nh_q_sensor_pose(v3(s.position), q4(s.rotation), mounted, exists, bp, bq);
	const nh_QSensorRay r = nh_q_sensor_ray(w, exists, v3(b.direction), b.range, s.ignore_body);
	nh_Ray out;
	out.origin[0] = r.o.x; out.origin[1] = r.o.y; out.origin[2] = r.o.z; out.max_t = r.max_t;
	out.direction[0] = r.d.x; out.direction[1] = r.d.y; out.direction[2] = r.d.z; out.ignore_body = r.ignore;
	return out;
}

}

extern "C" {

void hs_sense_rays(const nh_Sensor* sensors, uint32_t count, const nh_Beam* beams, uint32_t beam_count, const nh_Transform* bodies, uint32_t nbodies,
                   nh_Ray* rays, uint32_t threads) {
	parallel(count, threads, [=](uint32_t s) {
		for (uint32_t j = 0; j < beam_count; ++j) rays[(size_t)s * beam_count + j] = ray_of(sensors[s], beams[j], bodies, nbodies);
	});
}

// filter == 0: no mask is read.  Otherwise sensor s sees collider c iff (words[c] & m) != 0, m = masks[s] (masks null: `mask`); words null: all ones
void hs_sense(const Rec* rec, uint32_t n, uint32_t nbox, const nh_Sensor* sensors, uint32_t count, const nh_Beam* beams, uint32_t beam_count,
              const nh_Transform* bodies, uint32_t nbodies, uint32_t filter, const uint32_t* words, const uint32_t* masks, uint32_t mask,
              float* t, uint32_t* body, uint32_t* tag, nh_RayHit* hits, uint32_t threads) {
	std::vector<uint32_t> ones;
	if (filter && !words) { ones.assign(n, 0xffffffffu); words = ones.data(); }
	if (!filter) words = nullptr;
	parallel(count, threads, [=](uint32_t s) {
		for (uint32_t j = 0; j < beam_count; ++j) {
			const size_t i = (size_t)s * beam_count + j;
			const nh_Ray r = ray_of(sensors[s], beams[j], bodies, nbodies);
			float bt; uint32_t bc; nh_f3 bn;
			const bool ok = closest_hit(rec, n, nbox, SweptRay{}, v3(r.origin), v3(r.direction), r.max_t, r.ignore_body, words, masks ? masks[s] : mask, -1, bt, bc, bn);
			nh_RayHit h;
			write_cast(h, rec, nbox, ok, r.max_t, bt, bc, bn);
			if (t) t[i] = h.t;
			if (body) body[i] = h.body;
			if (tag) tag[i] = h.tag;
			if (hits) hits[i] = h;
		}
	});
}

}
