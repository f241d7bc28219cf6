// hostjoint.cpp -- CPU build of the per-item functions of the joints (nudge_amd/csrc/nh_joint.h), the oracle of the GPU's level-parallel replay
// (tests/hostjoint_util.py).  Everything here is serial and in the caller's list order, which is the specification:
//   hj_prepare       plain loops: the offsets' rules, the owner check assembly by assembly, then per bin the level rule straight from its definition (the last
//                    earlier valid joint that names a body, kept in a table per body) and a stable sort by level
//   hj_setup         for each joint in list order: live?  then the rows into the caller's solve records, the warm start row by row
//   hj_apply         `iterations` times: for each joint in list order, for each row in row order, one visit; then the accumulated impulses
//   hj_connections   the body pair of every valid joint, (0, 0) otherwise
//   hj_gravity, hj_advance   nh_solver.h's nh_gravity_damping / nh_advance_body over an active list (the sample's caller-side loop and nh_advance)
#include <algorithm>
#include <string.h>
#include "oracle.h"
#include "../../nudge_amd/csrc/nh_joint.h"

extern "C" {

uint32_t hj_solve_bytes() { return (uint32_t)sizeof(nh_JSolve); }

void hj_prepare(const nh_Joint* joints, uint32_t count, const uint32_t* offsets, uint32_t assemblies, uint32_t body_count, uint32_t* status,
                uint32_t* levels, uint32_t* order) {
	status[0] = status[1] = status[2] = status[3] = 0u;
	for (uint32_t j = 0u; j < count; ++j) { levels[j] = 0u; order[j] = j; }
	if (count == 0u) return;
	const uint32_t A = offsets ? assemblies : 1u;
	std::vector<uint32_t> off(A + 1u);
	for (uint32_t i = 0u; i <= A; ++i) off[i] = offsets ? offsets[i] : (i == 0u ? 0u : count);
	if (off[0] != 0u || off[A] != count) status[0] |= NH_JOINT_ERR_OFFSETS;
	for (uint32_t i = 0u; i < A; ++i) {
		if (off[i + 1u] < off[i]) status[0] |= NH_JOINT_ERR_OFFSETS;
		else if (off[i + 1u] - off[i] > NH_JOINT_ASSEMBLY_MAX) status[0] |= NH_JOINT_ERR_ASSEMBLY_SIZE;
	}
	for (uint32_t j = 0u; j < count; ++j) if (nh_j_valid(joints[j], body_count)) ++status[1];
	if (!(status[0] & NH_JOINT_ERR_OFFSETS)) {
		std::vector<uint32_t> owner(body_count, 0xFFFFFFFFu);
		for (int pass = 0; pass < 2; ++pass)
			for (uint32_t i = 0u; i < A; ++i)
				for (uint32_t j = off[i]; j < off[i + 1u]; ++j) {
					if (!nh_j_valid(joints[j], body_count)) continue;
					const uint32_t bin = off[i] / NH_JOINT_BIN, ab[2] = { joints[j].a, joints[j].b };
					for (uint32_t x : ab) {
						if (!x) continue;
						if (pass == 0) owner[x] = std::min(owner[x], bin);
						else if (owner[x] != bin) status[0] |= NH_JOINT_ERR_SHARED_BODY;
					}
				}
	}
	if (status[0]) return;
	std::vector<int64_t> last(body_count, -1);
	for (uint32_t w = 0u; w < (count + NH_JOINT_BIN - 1u) / NH_JOINT_BIN; ++w) {
		std::vector<uint32_t> span;
		for (uint32_t i = 0u; i < A; ++i)
			if (off[i] / NH_JOINT_BIN == w) for (uint32_t j = off[i]; j < off[i + 1u]; ++j) span.push_back(j);
		if (span.empty()) continue;
		++status[3];
		for (uint32_t j : span) {
			if (!nh_j_valid(joints[j], body_count)) continue;
			uint32_t l = 0u;
			const uint32_t ab[2] = { joints[j].a, joints[j].b };
			for (uint32_t x : ab) if (x && last[x] >= 0) l = std::max(l, levels[last[x]]);
			levels[j] = l + 1u;
			for (uint32_t x : ab) if (x) last[x] = j;
			status[2] = std::max(status[2], levels[j]);
		}
		for (uint32_t j : span) { if (joints[j].a < body_count) last[joints[j].a] = -1; if (joints[j].b < body_count) last[joints[j].b] = -1; }
		std::vector<uint32_t> sorted = span;
		std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t x, uint32_t y) { return levels[x] < levels[y]; });
		for (size_t k = 0; k < span.size(); ++k) order[span[0] + k] = sorted[k];
	}
}

// momentum is changed IN PLACE (the caller passes a copy) and moved as bytes: unused0 / unused1 keep their bits.  `solve`: count records of hj_solve_bytes().
void hj_setup(const nh_Transform* transforms, const nh_BodyProperties* properties, nh_BodyMomentum* momentum, uint32_t body_count, const uint32_t* active,
              uint32_t active_count, const nh_Joint* joints, uint32_t count, uint32_t status0, const nh_JointParams* params, const nh_JointImpulse* impulses,
              nh_JSolve* solve) {
	if (status0) return;
	std::vector<uint8_t> live(body_count, 0u);
	for (uint32_t k = 0u; k < active_count; ++k) if (active[k] < body_count) live[active[k]] = 1u;
	for (uint32_t jx = 0u; jx < count; ++jx) {
		const nh_Joint& j = joints[jx];
		nh_JSolve& s = solve[jx];
		s.head = nh_JHead{ j.a, j.b, 0u, j.type, 0.0f, 0.0f, { 0.0f, 0.0f } };
		if (!(nh_j_valid(j, body_count) && ((j.a && live[j.a]) || (j.b && live[j.b])))) continue;
		const nh_JSide A = nh_j_side(j.a, transforms[j.a], properties[j.a]), B = nh_j_side(j.b, transforms[j.b], properties[j.b]);
		const nh_JFrame f = nh_j_frame(j, A, B);
		nh_JMom ma = nh_j_zero_mom(), mb = nh_j_zero_mom();
		if (j.a) memcpy(&ma, momentum + j.a, sizeof(ma));
		if (j.b) memcpy(&mb, momentum + j.b, sizeof(mb));
		const uint32_t rows = nh_j_rows(j.type);
		for (uint32_t k = 0u; k < rows; ++k) {
			bool dead;
			nh_JRow r = nh_j_row(j, k, f, A, B, *params, &dead);
			r.acc = dead ? 0.0f : params->warm * impulses[jx].row[k];
			nh_j_push(r, nh_j_linear(j.type, k), r.acc, A.mi, B.mi, ma, mb);
			s.row[k] = r;
		}
		if (j.a) memcpy(momentum + j.a, &ma, sizeof(ma));
		if (j.b) memcpy(momentum + j.b, &mb, sizeof(mb));
		s.head.rows = rows; s.head.mi_a = A.mi; s.head.mi_b = B.mi;
	}
}

void hj_apply(nh_BodyMomentum* momentum, uint32_t body_count, uint32_t count, uint32_t status0, nh_JSolve* solve, nh_JointImpulse* impulses, uint32_t iterations) {
	if (status0) return;
	for (uint32_t it = 0u; it < iterations; ++it)
		for (uint32_t jx = 0u; jx < count; ++jx) {
			nh_JSolve& s = solve[jx];
			const nh_JHead& h = s.head;
			if (h.rows == 0u || h.rows > NH_JOINT_ROWS_MAX || h.a >= body_count || h.b >= body_count) continue;
			nh_JMom ma = nh_j_zero_mom(), mb = nh_j_zero_mom();
			if (h.a) memcpy(&ma, momentum + h.a, sizeof(ma));
			if (h.b) memcpy(&mb, momentum + h.b, sizeof(mb));
			for (uint32_t k = 0u; k < h.rows; ++k) nh_j_visit(s.row[k], nh_j_linear(h.type, k), h.mi_a, h.mi_b, ma, mb);
			if (h.a) memcpy(momentum + h.a, &ma, sizeof(ma));
			if (h.b) memcpy(momentum + h.b, &mb, sizeof(mb));
			if (it + 1u == iterations) {
				nh_JointImpulse out;
				memset(&out, 0, sizeof(out));
				for (uint32_t k = 0u; k < h.rows; ++k) out.row[k] = s.row[k].acc;
				impulses[jx] = out;
			}
		}
}

void hj_connections(const nh_Joint* joints, uint32_t count, uint32_t body_count, nh_BodyPair* out) {
	for (uint32_t j = 0u; j < count; ++j) {
		const bool ok = nh_j_valid(joints[j], body_count);
		out[j] = nh_BodyPair{ ok ? joints[j].a : 0u, ok ? joints[j].b : 0u };
	}
}

void hj_gravity(nh_BodyMomentum* momentum, const uint32_t* active, uint32_t active_count, float gx_dt, float gy_dt, float gz_dt, float damping) {
	for (uint32_t k = 0u; k < active_count; ++k) {
		nh_BodyMomentum& m = momentum[active[k]];
		nh_gravity_damping(m.velocity, m.angular_velocity, gx_dt, gy_dt, gz_dt, damping);
	}
}

void hj_advance(nh_Transform* transforms, const nh_BodyMomentum* momentum, uint8_t* idle, const uint32_t* active, uint32_t active_count, float time_step) {
	for (uint32_t k = 0u; k < active_count; ++k) {
		const uint32_t i = active[k];
		idle[i] = nh_advance_body(transforms[i].position, transforms[i].rotation, momentum[i].velocity, momentum[i].angular_velocity, idle[i], time_step);
	}
}

}
