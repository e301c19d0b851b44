// Part of the Mitsuba plugin `drmlt.so` (mitsuba_adaptor.cpp includes it, after the Mitsuba headers and drmlt_abi.h): the
// emitters of a scene that no shape carries. These are the plugin's calls into Mitsuba's API beyond what
// tests/native/fake_mitsuba/ declares; the development image compiles the plugin against tests/native/fake_mitsuba_emitters/
// (that header plus the declarations used here). tests/test_fake_mitsuba_emitters_signatures.py runs the checks of
// tests/test_fake_mitsuba_signatures.py over mitsuba_adaptor.cpp and this file together, against that header.
#pragma once

#include <cstring>
#include <string>
#include <vector>

MTS_NAMESPACE_BEGIN

// Emitters that no shape carries (scene.h:1113-1115); the adaptor's appendShape has turned the area lights into `emitters`
// already, in shape order, the lights of the k-th emitting shape ending at lightEnds[k]. The emitters' order is the order of
// the sampling distribution (drmlt_abi.h), and Mitsuba builds that over Scene::m_emitters in its own order
// (scene.cpp:385-390). So a free emitter is placed behind as many emitting shapes' lights as m_emitters holds shape-carried
// emitters in front of it; the area lights keep shape order among themselves. (A scene loaded from XML has its free emitters
// in front of every area light: addChild appends them while the file is read, scene.cpp:547-567, and initialize() appends
// the shapes' emitters afterwards, :332-347 and :621-622.) A scene without free emitters is left exactly as appendShape made it.
inline void appendEmitters(const Scene *scene, std::vector<drmlt_emitter> &emitters, std::vector<float> &points,
                           std::vector<drmlt_shape> &shapes, const std::vector<size_t> &lightEnds) {
    const ref_vector<Emitter> &mtsEmitters = scene->getEmitters();
    std::vector<drmlt_emitter> ordered;
    size_t carried = 0, placed = 0, nFree = 0; // shape-carried emitters seen; emitting shapes whose lights are placed
    auto placeLights = [&](size_t upto) {
        for (; placed < upto && placed < lightEnds.size(); ++placed)
            for (size_t i = placed ? lightEnds[placed - 1] : 0; i < lightEnds[placed]; ++i) {
                shapes[emitters[i].shape].emitter = (int32_t) ordered.size();
                ordered.push_back(emitters[i]);
            }
    };
    for (size_t i = 0; i < mtsEmitters.size(); ++i) {
        const Emitter *em = mtsEmitters[i].get();
        if (em->getShape() != NULL) { ++carried; continue; }
        std::string name = em->getClass()->getName();
        drmlt_emitter e;
        memset(&e, 0, sizeof e);
        Float r = 0, g = 0, b = 0;
        if (name == "PointEmitter") { // point.cpp:57-69; the position as sampleDirect finds it, :131-134
            e.type = DRMLT_EMITTER_POINT;
            e.shape = (int32_t) (points.size() / 3);
            const Point p = em->getWorldTransform()->eval(0).transformAffine(Point(0.0f, 0.0f, 0.0f));
            points.push_back((float) p.x); points.push_back((float) p.y); points.push_back((float) p.z);
            em->getProperties().getSpectrum("intensity", Spectrum::getD65()).toLinearRGB(r, g, b);
        } else if (name == "ConstantBackgroundEmitter") { // constant.cpp:47-50
            e.type = DRMLT_EMITTER_CONSTANT;
            e.shape = -1;
            em->getProperties().getSpectrum("radiance", Spectrum::getD65()).toLinearRGB(r, g, b);
        } else {
            SLog(EError, "Emitter type %s has no MI355X drmlt implementation (refusing rather than approximating)", name.c_str());
        }
        e.radiance[0] = (float) r; e.radiance[1] = (float) g; e.radiance[2] = (float) b;
        e.sampling_weight = (float) em->getSamplingWeight();
        placeLights(carried);
        ordered.push_back(e);
        ++nFree;
    }
    if (nFree == 0) return;
    placeLights(lightEnds.size());
    emitters = ordered;
}

MTS_NAMESPACE_END
