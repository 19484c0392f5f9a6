// TEST INFRASTRUCTURE — NOT PART OF THE PRODUCT. Compiled by tests/test_additive_compress_oracle.py into a temporary directory, never
// committed as a binary; skipped where the reference's sources are absent.
//
// The reference's own compressor (its headers, read in place, against oracle/rtm_shim/) called with AN ADDITIVE BASE:
// compress_track_list(allocator, track_list, settings, additive_base_track_list, additive_format, ...) with the variable formats and
// the matching additive_qvvf_transform_error_metric<format>. oracle/ref_compress_bridge.cpp has no base argument; this is that call
// with two track arrays.
#include <acl/core/additive_utils.h>
#include <acl/core/ansi_allocator.h>
#include <acl/core/compressed_tracks.h>
#include <acl/compression/compress.h>
#include <acl/compression/compression_settings.h>
#include <acl/compression/track_array.h>
#include <acl/compression/transform_error_metrics.h>

#include <cstdint>
#include <cstring>
#include <utility>

namespace
{
	// samples: [num_samples][num_tracks][12] floats (rotation xyzw | translation xyz_ | scale xyz_); parents: -1 is a root, or null;
	// bind_pose: [num_tracks][12] or null (the identity)
	void fill(acl::iallocator& allocator, acl::track_array_qvvf& tracks, const float* samples, uint32_t num_tracks, uint32_t num_samples, float sample_rate,
		const int32_t* parents, const float* bind_pose, float precision, float shell_distance)
	{
		for (uint32_t track_index = 0; track_index < num_tracks; ++track_index)
		{
			acl::track_desc_transformf desc;
			desc.output_index = track_index;
			desc.parent_index = parents != nullptr && parents[track_index] >= 0 ? uint32_t(parents[track_index]) : acl::k_invalid_track_index;
			desc.precision = precision;
			desc.shell_distance = shell_distance;
			if (bind_pose != nullptr)
			{
				const float* qvv = bind_pose + size_t(track_index) * 12;
				desc.default_value = rtm::qvv_set(rtm::quat_load(qvv + 0), rtm::vector_load3(qvv + 4), rtm::vector_load3(qvv + 8));
			}
			acl::track_qvvf track = acl::track_qvvf::make_reserve(desc, allocator, num_samples, sample_rate);
			for (uint32_t sample_index = 0; sample_index < num_samples; ++sample_index)
			{
				const float* qvv = samples + (size_t(sample_index) * num_tracks + track_index) * 12;
				track[sample_index] = rtm::qvv_set(rtm::quat_load(qvv + 0), rtm::vector_load3(qvv + 4), rtm::vector_load3(qvv + 8));
			}
			tracks[track_index] = std::move(track);
		}
	}
}

// additive_format: acl::additive_clip_format8 (0: the call without a base); level: acl::compression_level8; flags: bit 0 optimize_loops.
// Returns the blob's size, 0 on error (the message in `error`); the blob is copied into `out` when it fits.
extern "C" uint32_t aclref_compress_additive(const float* samples, uint32_t num_tracks, uint32_t num_samples, float sample_rate, const float* base_samples,
	uint32_t base_num_tracks, uint32_t base_num_samples, float base_sample_rate, uint32_t additive_format, const int32_t* parents, const float* bind_pose, uint32_t level,
	uint32_t flags, float precision, float shell_distance, void* out, uint32_t capacity, char* error, uint32_t error_capacity)
{
	acl::ansi_allocator allocator;
	uint32_t size = 0;
	{
		acl::track_array_qvvf tracks(allocator, num_tracks), base(allocator, base_num_tracks);
		fill(allocator, tracks, samples, num_tracks, num_samples, sample_rate, parents, bind_pose, precision, shell_distance);
		fill(allocator, base, base_samples, base_num_tracks, base_num_samples, base_sample_rate, nullptr, nullptr, precision, shell_distance);

		acl::compression_settings settings;
		settings.level = static_cast<acl::compression_level8>(level);
		settings.rotation_format = acl::rotation_format8::quatf_drop_w_variable;
		settings.translation_format = acl::vector_format8::vector3f_variable;
		settings.scale_format = acl::vector_format8::vector3f_variable;
		acl::qvvf_transform_error_metric plain;
		acl::additive_qvvf_transform_error_metric<acl::additive_clip_format8::relative> relative;
		acl::additive_qvvf_transform_error_metric<acl::additive_clip_format8::additive0> additive0;
		acl::additive_qvvf_transform_error_metric<acl::additive_clip_format8::additive1> additive1;
		acl::itransform_error_metric* metrics[4] = { &plain, &relative, &additive0, &additive1 };
		settings.error_metric = metrics[additive_format & 3u];
		settings.optimize_loops = (flags & 1u) != 0;

		acl::output_stats stats;
		acl::compressed_tracks* compressed = nullptr;
		const acl::error_result result = additive_format == 0 ? acl::compress_track_list(allocator, tracks, settings, compressed, stats)
			: acl::compress_track_list(allocator, tracks, settings, base, static_cast<acl::additive_clip_format8>(additive_format), compressed, stats);
		if (result.any() || compressed == nullptr)
		{
			if (error != nullptr && error_capacity != 0)
			{
				std::strncpy(error, result.c_str(), error_capacity - 1);
				error[error_capacity - 1] = '\0';
			}
			return 0;
		}
		size = compressed->get_size();
		if (out != nullptr && capacity >= size)
			std::memcpy(out, compressed, size);
		allocator.deallocate(compressed, size);
	}
	return size;
}
